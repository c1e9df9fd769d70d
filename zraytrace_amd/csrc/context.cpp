// context.cpp - the device-resident scene behind zrt_ctx_*: creation and upload,
// the frame launch (render, accumulation pass, adaptive level) with its scheduling
// probe, launch status, stats, scanlines and the assemble calls.  The run entry
// points: runs.cpp; features, denoise, temporal: post.cpp; zrt_trace and the debug
// entry points that run a kernel: debug_device.cpp.  The kernels: render.hip.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "accel_build.hpp"
#include "context.hpp"

namespace zrt {
static const KernelConfig& K = kernel_config();

int check_device(int dev) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
    return fail(ZRT_E_NODEVICE, "no HIP device visible (the HIP path needs an MI355X / gfx950)");
  if (dev < 0 || dev >= count) return fail(ZRT_E_NODEVICE, "device ordinal out of range");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return fail(ZRT_E_NODEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(ZRT_E_NODEVICE, std::string("device is ") + prop.gcnArchName + ", libzrt is built for gfx950 only");
  return ZRT_OK;
}

void flatten_for_device(HostScene* h, const zrt_scene* s, bool use_bvh, int device) {
  flatten_scene(h, s, use_bvh, device);
  if (h->device_bvh_failed) (void)hipGetLastError();
}

// Upload a flattened scene to the context's device.
static void upload_scene(Scene& s, const HostScene& h) {
  const double t1 = now_ms();
  s.nodes.upload(h.nodes);
  s.wnodes.upload(h.wn);
  if (h.q_ok) {
    s.qnodes.upload(h.qn);
    s.qleaves.upload(h.ql);
  }
  s.q_stride = h.q_stride;
  s.n_qleaves = uint32_t(h.ql.size() / kLeafRecF4);
  s.prims.upload(h.prims);
  s.shade.upload(h.shade);
  s.mats.upload(h.mats);
  s.texels.upload(h.tex);
  s.texels8.upload(h.tex8);
  s.leaf_of_slot.upload(h.leaf_of_slot);
  s.ref_sph.upload(h.ref_sph);
  for (int k = 0; k < 3; ++k) s.root_c[k] = h.root_c[k];
  s.origin_bound = h.origin_bound;
  s.layout = h.layout;
  s.graze_m = h.graze_m;
  s.graze_leaf = h.graze_leaf;
  s.upload_ms = now_ms() - t1;
  s.preprocess_ms = h.preprocess_ms;
  s.n_prims = h.n_prims;
  s.bvh_depth = h.bvh_depth;
  s.wide_stride = h.wide_stride;
  s.texel_bytes = h.texel_bytes;
  s.tri_rcp_fast = h.tri_rcp_fast;
  s.scene_extent = h.scene_extent;
  for (int k = 0; k < 3; ++k) {
    s.tri_c[k] = h.tri_c[k];
    s.tri_h[k] = h.tri_h[k];
  }
  s.slot_to_prim = h.slot_to_prim;
  s.shape = shape_of(h);
}

// ---- KArgs, filled once (kernels.hpp): each launch adds only what is its own ----
// The tree a launch traverses: the full wide nodes, or (qn) the compressed ones.
static void fill_tree(KArgs& a, const Scene& s, bool qn) {
  a.wnodes = qn ? s.qnodes.p : s.wnodes.p;
  a.wide_stride = qn ? s.q_stride : s.wide_stride;
  a.node_f4 = qn ? kQuantNodeF4 : 8u;
  a.qleaves = qn ? s.qleaves.p : nullptr;
  a.n_qnodes = qn ? s.q_stride / kQuantNodeF4 : 0u;
  a.n_qleaves = qn ? s.n_qleaves : 0u;
  a.n_top = qn ? s.shape.q_top : s.shape.n_top;
}
// The scene part: the context's buffers and constants, its error flag, and the
// traversal stack's depth (the reference traversal's rows: at most its own).
static void fill_scene(KArgs& a, const zrt_ctx* c, bool qn, uint32_t stack_depth) {
  const Scene& s = c->scene;
  a.nodes = s.nodes.p;
  a.prims = s.prims.p;
  a.shade = s.shade.p;
  a.mats = s.mats.p;
  a.texels = s.texels.p;
  a.texels8 = s.texels8.p;
  a.n_mats = s.shape.n_mats;
  fill_tree(a, s, qn);
  a.error_flag = reinterpret_cast<uint32_t*>(c->scratch.p + kErrorSlot);
  a.n_list = s.shape.use_bvh ? 0 : s.n_prims;
  a.tri_rcp_fast = s.tri_rcp_fast;
  a.scene_extent = s.scene_extent;
  a.paxis_m = paxis_threshold();
  for (int k = 0; k < 3; ++k) {
    a.tri_c[k] = s.tri_c[k];
    a.tri_h[k] = s.tri_h[k];
    a.root_c[k] = s.root_c[k];
  }
  a.stack_depth = stack_depth;
  a.ref_stack = std::min(s.shape.stack_depth, stack_depth);
  a.leaf_of_slot = s.leaf_of_slot.p;
  a.ref_sph = s.ref_sph.p;
  a.origin_bound = s.origin_bound;
  a.layout = s.layout;
  a.graze_m = s.graze_m;
  a.graze_leaf = s.graze_leaf;
}
// The camera and the frame's size.
void fill_camera(KArgs& a, const zrt_camera* cam, const zrt_params* p) {
  copy3(a.org, cam->origin);
  copy3(a.llc, cam->lower_left_corner);
  copy3(a.hor, cam->horizontal);
  copy3(a.ver, cam->vertical);
  a.f_width = float(p->width);
  a.f_height = float(p->height);
  a.inv_width = 1.0f / a.f_width;  // IEEE RN(1/width): dev::div_core's y
  a.inv_height = 1.0f / a.f_height;
  a.width = p->width;
  a.height = p->height;
  a.xbound = geometry(p).xbound;
}
// The block's LDS regions.
static void fill_lds(KArgs& a, const LdsPlan& lp) {
  a.lds_rows = lp.stack_rows;
  a.lds_top_off = lp.top_off;
  a.lds_att_off = lp.att_off;
  a.att_lds_rows = lp.att_rows;
  a.lds_mat_off = lp.mat_off;
  a.mats_in_lds = lp.mats_in_lds;
  a.lds_pool_off = lp.pool_off;
  a.lds_state_off = lp.state_off;
}

// The launch of zrt_trace and zrt_ctx_features: one lane per ray over the loop's own
// traversal (FAST: over the compressed nodes where the context built them, MODE 8),
// with the grazing-triangle guard, any ray origin and no attenuation rows (max_depth 0;
// the radiance query plans rows for its paths).
TracePlan fill_trace(KArgs& a, const zrt_ctx* c, uint32_t traversal, bool full_nodes, uint32_t max_depth) {
  const Scene& s = c->scene;
  const int mode = !s.shape.use_bvh ? 0 : traversal == ZRT_TRAVERSAL_REFERENCE ? 2 : traversal == ZRT_TRAVERSAL_BINARY ? 1 : 3;
  const uint32_t stack_depth = mode == 3 ? std::max(s.shape.wide_stack, s.shape.stack_depth) : s.shape.stack_depth;
  const bool qn = mode == 3 && s.shape.q_ok && !full_nodes;
  TracePlan t;
  t.kmode = qn ? 8 : mode;
  t.stk16 = mode == 3 ? fast_stk16(s.shape.n_wide, s.shape.n_nodes) : s.shape.n_nodes < 65536;
  t.lp = plan_lds(qn ? s.shape.q_top : s.shape.n_top, s.shape.n_mats, mode, t.stk16, stack_depth, max_depth, false, false,
                  ZRT_PRNG_XOROSHIRO128, qn ? kQuantNodeF4 : 8u);
  fill_scene(a, c, qn, stack_depth);
  fill_lds(a, t.lp);
  a.check_origins = 1;
  a.guard = s.shape.guard;
  return t;
}
const uint32_t* slot_prim_table(zrt_ctx* c) {
  Scene& s = c->scene;
  if (s.slot_prim.n < s.slot_to_prim.size() || s.slot_prim.p == nullptr) s.slot_prim.upload(s.slot_to_prim);
  return s.slot_prim.p;
}
// Its deep stack rows in `ovf`, grown once `st` has drained (an earlier launch may
// still use the old rows), and the bounds the STATS check would read.
void trace_rows(KArgs& a, const zrt_ctx* c, const TracePlan& t, uint64_t n_lanes, DevBuf<uint8_t>& ovf, hipStream_t st,
                const char* launch) {
  a.n_lanes = uint32_t(n_lanes);
  const BufNeed need = buffer_need(t.lp, 0, a.stack_depth, n_lanes, n_lanes, t.stk16);
  if (need.ovf_bytes) {
    if (ovf.n < need.ovf_bytes) {
      HIPCHK(hipStreamSynchronize(st));
      ovf.alloc(need.ovf_bytes);
    }
    a.stack_ovf = ovf.p;
  }
  check_buffers(launch, BufNeed{0, need.ovf_bytes}, c->att.n, ovf.n);
  a.att_cap = c->att.n;
  a.ovf_cap = ovf_cap_elems(ovf.n, t.stk16);
}

// Longest-processing-time-first order of this rank's tiles (zrt.h,
// ZRT_FLAG_NO_SCHEDULE): the probe renders K.probe_spp samples of every tile as
// one unit each and records the loop iterations its wave spent (lockstep makes
// that the unit's time); a stable device radix sort orders the tiles by
// descending cost, ties in tile order.  Sets a.tile_order for the render launch.
static bool schedule_tiles(zrt_ctx* c, KArgs& a, uint32_t prng, bool stk16, uint32_t my_tiles, uint32_t grid,
                           hipStream_t st) {
  Probe& pr = c->probe;
  // the probe is the lockstep loop over the full nodes, whatever loop and node
  // format the render launch uses: its own LDS plan (the render's may be the path
  // pool's, whose regions the lockstep loop would read as its lane state and rows)
  const SceneShape& sh = c->scene.shape;
  const LdsPlan pp = plan_lds(sh.n_top, sh.n_mats, 3, stk16, a.stack_depth, a.max_depth, false, false, prng);
  // (it reads the material table from LDS only: no schedule for a table past its LDS
  // share - the render then takes the tiles in order)
  if (!pp.mats_in_lds) return false;
  pr.partial.grow(uint64_t(my_tiles) * 64u);
  pr.scratch.grow(kScratchSlots);
  if (pr.tile_cost.n < my_tiles) {
    pr.tile_cost.alloc(my_tiles);
    pr.cost_sorted.alloc(my_tiles);
    pr.tile_order.alloc(my_tiles);
  }
  if (pr.tile_ids_n != my_tiles) {
    std::vector<uint32_t> ids(my_tiles);
    for (uint32_t i = 0; i < my_tiles; ++i) ids[i] = i;
    pr.tile_ids.upload(ids);
    pr.tile_ids_n = my_tiles;
  }
  // the render launch's arguments, but: one unit of K.probe_spp samples per tile in
  // tile order, its cost recorded; the probe's own sums and counters (the error flag
  // stays the render's: a probe overflow fails the frame too); the full nodes and the
  // lockstep loop's LDS plan
  KArgs pa = a;
  pa.spp = pa.chunk = K.probe_spp;
  pa.n_chunks = 1;
  pa.total_work = my_tiles;
  pa.tile_order = nullptr;
  pa.unit_cost = pr.tile_cost.p;
  pa.partial = pr.partial.p;
  pa.counters = pr.scratch.p;
  pa.work_counter = reinterpret_cast<uint32_t*>(pr.scratch.p + kWorkSlot);
  const uint32_t pgrid = std::max(1u, std::min(grid, (my_tiles + kBlock / 64 - 1) / (kBlock / 64)));
  pa.n_lanes = pgrid * kBlock;
  fill_tree(pa, c->scene, false);
  fill_lds(pa, pp);
  // its deep stack rows and global attenuation rows ([row][lane] past its LDS rows):
  // the render launch's buffers, grown if the probe's plan needs more (the wavefront
  // loop keeps 12 attenuation rows in LDS, the lockstep probe 4)
  const BufNeed need = buffer_need(pp, a.max_depth, a.stack_depth, pa.n_lanes, pa.n_lanes, stk16);
  if (need.ovf_bytes) {
    if (c->stack_ovf.n < need.ovf_bytes) {
      HIPCHK(hipStreamSynchronize(st));  // (the previous launch may still read the old buffer)
      c->stack_ovf.alloc(need.ovf_bytes);
    }
    a.stack_ovf = pa.stack_ovf = c->stack_ovf.p;
  }
  if (c->att.n < need.att_elems) {
    HIPCHK(hipStreamSynchronize(st));  // (the previous launch may still read the old buffer)
    c->att.alloc(need.att_elems);
  }
  a.att = pa.att = c->att.p;
  a.att_cap = pa.att_cap = c->att.n;
  a.ovf_cap = pa.ovf_cap = ovf_cap_elems(c->stack_ovf.n, stk16);
  check_buffers("scheduling probe", need, c->att.n, c->stack_ovf.n);
  HIPCHK(hipMemsetAsync(pr.scratch.p, 0, kScratchSlots * sizeof(unsigned long long), st));
  void* args[] = {&pa};
  HIPCHK(hipLaunchKernel(probe_kernel(prng, stk16), dim3(pgrid), dim3(kBlock), args, pp.bytes, st));
  size_t bytes = 0;
  HIPCHK(sort_tiles(nullptr, &bytes, pr.tile_cost.p, pr.cost_sorted.p, pr.tile_ids.p, pr.tile_order.p, my_tiles, st));
  pr.sort_temp.grow(bytes);
  HIPCHK(sort_tiles(pr.sort_temp.p, &bytes, pr.tile_cost.p, pr.cost_sorted.p, pr.tile_ids.p, pr.tile_order.p, my_tiles,
                    st));
  a.tile_order = pr.tile_order.p;
  ++pr.order_gen;
  return true;
}

int hip_fail(const HipError& e) {
  return fail(ZRT_E_HIP, e.where + ": " + hipGetErrorString(e.err));
}

constexpr const char* kOverflowMsg = "BVH traversal stack overflow (tree deeper than the stack was sized for)";
constexpr const char* kLayoutMsg = "the kernel refused the wide tree: its layout is not the one the kernel decodes";
constexpr const char* kBoundsMsg = "a global attenuation or stack row index past its buffer (STATS bounds check)";
const char* device_error_msg(unsigned long long flag) {
  return (flag & kErrLayout) ? kLayoutMsg : (flag & kErrBounds) ? kBoundsMsg : kOverflowMsg;
}

// One launch's device error.  wait: block until the launch is done; else look only
// if it has finished (a launch still running is no error, and leaves none behind in
// HIP).  An error already returned to the caller is returned again only by a
// waiting call, and (once) not even by that.
static int completion_status(Completion& k, bool wait, bool once) {
  if (!k.launched || (k.reported && (once || !wait))) return ZRT_OK;
  if (wait) {
    HIPCHK(hipEventSynchronize(k.done));
  } else if (hipEventQuery(k.done) != hipSuccess) {
    (void)hipGetLastError();
    return ZRT_OK;
  }
  if (*k.err == 0) return ZRT_OK;
  k.reported = true;
  return fail(ZRT_E_UNSUPPORTED, device_error_msg(*k.err));
}
// The device errors of the context's launches: a feature launch's first, then a ray
// query's, each reported once; then the last render launch's - every waiting call
// reports it, render_tiles' sticky check (wait false) only until some call has.
int launch_status(zrt_ctx* c, bool wait) {
  int rc = completion_status(c->feat.done, wait, true);
  if (!rc) rc = completion_status(c->query.done, wait, true);
  return rc ? rc : completion_status(c->render, wait, false);
}

LaunchTimes launch_times(const EvSet& e) {
  LaunchTimes t{};
  HIPCHK(hipEventElapsedTime(&t.render_ms, e.pre, e.e1));
  HIPCHK(hipEventElapsedTime(&t.schedule_ms, e.pre, e.e0));
  HIPCHK(hipEventElapsedTime(&t.kernel_ms, e.e0, e.e1));
  if (!e.probed) t.schedule_ms = 0.0f;  // (also when a kept order was reused)
  return t;
}

// A run's earlier passes whose events have completed (wait: all of them) added into
// its render and schedule times; their event sets become spare.  Passes complete in
// the order they were enqueued.
void fold_pass_times(zrt_ctx* c, bool wait) {
  AccumRun& r = c->run;
  while (!r.pending.empty()) {
    EvSet& e = r.pending.front();
    if (wait) {
      HIPCHK(hipEventSynchronize(e.e1));
    } else if (hipEventQuery(e.e1) != hipSuccess) {
      (void)hipGetLastError();  // (not ready is no error of this launch)
      break;
    }
    const LaunchTimes t = launch_times(e);
    r.render_ms += t.render_ms;
    r.sched_ms += t.schedule_ms;
    r.spare.push_back(std::move(e));
    r.pending.erase(r.pending.begin());
  }
}

// A context on `device` holding an uploaded copy of a flattened scene.
std::unique_ptr<zrt_ctx> ctx_on_device(const HostScene& h, int device) {
  std::unique_ptr<zrt_ctx> c(new zrt_ctx);
  c->device = device;
  HIPCHK(hipSetDevice(c->device));
  c->stream.create();
  c->ev.create();
  c->render.create();
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c->device));
  c->cu_count = prop.multiProcessorCount;
  upload_scene(c->scene, h);
  build_sky_scene(&c->sky.scene, h);
  c->scratch.alloc(kScratchSlots);
  return c;
}

// channels: 3 (the frame) or 1 (a plane, zrt_ctx_assemble_plane)
static int assemble(zrt_ctx* c, const zrt_params* p, const float* dev_gathered, uint32_t stride_tiles, float* dev_frame,
             void* hip_stream, uint32_t channels = 3) {
  if (!c || !dev_gathered || !dev_frame) return fail(ZRT_E_INVALID, "null argument");
  const int rc = validate_params(p);
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, hip_stream);
    const Geometry g = geometry(p);
    uint32_t total = 0;
    if (stride_tiles) {
      for (uint32_t r = 0; r < p->world_size; ++r)
        if (rank_tiles(g, r, p->world_size) > stride_tiles)
          return fail(ZRT_E_INVALID, "stride_tiles is smaller than a rank's tile count");
      if (uint64_t(stride_tiles) * 64u * p->world_size >= (1ull << 32)) return fail(ZRT_E_UNSUPPORTED, "frame too large");
      total = stride_tiles * 64u * p->world_size;
    } else {
      std::vector<uint32_t> base(p->world_size + 1, 0);
      for (uint32_t r = 0; r < p->world_size; ++r) base[r + 1] = base[r] + rank_tiles(g, r, p->world_size) * 64u;
      c->rank_base.upload(base);
      total = base[p->world_size];
    }
    HIPCHK(hipMemsetAsync(dev_frame, 0, sizeof(float) * channels * size_t(p->width) * p->height, st));
    if (total) {
      HIPCHK((channels == 1 ? launch_assemble_plane : launch_assemble)(
          st, dev_gathered, dev_frame, stride_tiles ? nullptr : c->rank_base.p, p->world_size, g.tiles_x, g.xbound,
          p->height, p->width, total, stride_tiles * 64u, g.n_tiles));
    }
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// Valid params (validate_params) are also the context's: its device, its BVH decision.
int params_fit_ctx(const zrt_ctx* c, const zrt_params* p) {
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  if ((p->bounded_volume_hierarchy != 0 && c->scene.n_prims > 10) != c->scene.shape.use_bvh)
    return fail(ZRT_E_INVALID,
                "params->bounded_volume_hierarchy implies another preprocessSufraces decision (raytrace.zig:124-133) "
                "than the one the context was built with");
  return ZRT_OK;
}

// ---- the frame launch, stage by stage (launch_frame) ----
namespace {
// The environment switches of a launch.  Read on every launch: tests change them
// between launches of one process.
struct LaunchEnv {
  bool debug = false;         // ZRT_DEBUG_LAUNCH: print the launch decision
  uint32_t wf_thresh = 48;    // ZRT_WF_THRESH: shade once 3/4 of the unit's active lanes are ready
                              // (C5: 32 -> 7.32, 48 -> 7.71, 56 -> 7.70 Gray/s)
  uint32_t sync = 0;          // ZRT_SYNC: A/B, the lockstep interval in samples (identical images); 0: unset
  bool order_cache = true;    // ZRT_ORDER_CACHE=0: A/B, probe every frame
  bool auto_sync = true;      // ZRT_SYNC or ZRT_AUTO_SYNC=0: the fixed interval, A/B
  bool sky_tiles = true;      // ZRT_SKY_TILES=0: A/B, every tile through the render kernel
  bool sky_by_render = false; // ZRT_SKY_TILES=2: measurement, the sky list through a second launch of the render kernel
  bool sphere_tiles = true;   // ZRT_SPHERE_TILES=0: A/B, the one-sphere tiles stay general
  bool sphere_by_render = false;  // ZRT_SPHERE_TILES=2: measurement, the one-sphere list through a launch of the render kernel
  bool cap_rows = false;      // ZRT_DEBUG_ROW_CAP: tests, the STATS device check reports a smaller buffer
  double row_cap = 1.0;
};
LaunchEnv read_launch_env() {
  LaunchEnv v;
  v.debug = std::getenv("ZRT_DEBUG_LAUNCH") != nullptr;
  if (const char* e = std::getenv("ZRT_WF_THRESH")) v.wf_thresh = uint32_t(std::max(1, std::min(64, std::atoi(e))));
  if (const char* e = std::getenv("ZRT_SYNC")) v.sync = std::max(1u, uint32_t(std::atoi(e)));
  const char* oc = std::getenv("ZRT_ORDER_CACHE");
  v.order_cache = !(oc && std::atoi(oc) == 0);
  const char* as = std::getenv("ZRT_AUTO_SYNC");
  v.auto_sync = !v.sync && !(as && std::atoi(as) == 0);
  v.sky_tiles = sky_tiles_wanted();
  if (const char* e = std::getenv("ZRT_SKY_TILES")) v.sky_by_render = std::atoi(e) == 2;
  v.sphere_tiles = sphere_tiles_wanted();
  if (const char* e = std::getenv("ZRT_SPHERE_TILES")) v.sphere_by_render = std::atoi(e) == 2;
  if (const char* e = std::getenv("ZRT_DEBUG_ROW_CAP")) {
    v.cap_rows = true;
    v.row_cap = std::atof(e);
  }
  return v;
}

// What one launch is: fixed by plan_frame, read by every later stage.
struct Frame {
  const zrt_camera* cam;
  const zrt_params* p;
  float* dev_tiles;
  hipStream_t st;
  // run_pass: a pass of the context's run (resolved by accumulate_kernel), not a whole frame
  // (finalize_kernel); first: the launch zeroes the counters it adds into; adapt: a level of
  // an adaptive run, the active tiles only; diag: ZRT_FLAG_STATS; cam_inside: the camera inside
  // the origin bound, and so every ray of the launch (scattered rays start at hits)
  bool run_pass, first, adapt, diag, cam_inside;
  zrt_pass_plan pass;
  Geometry g;
  uint32_t my_tiles;
  LaunchPlan plan;  // the launch decision (plan_launch; zrt_debug_launch_plan reports the same)
  void* kfn;
};
// The launch's extent: what occupancy and the work make of the plan.
struct FrameSize {
  int per_cu;
  // n_act: tiles the launch hands out; work: its units (tile, chunk), < 2^32 (plan_pass)
  uint32_t grid, n_act, work;
  uint64_t n_lanes, n_paths;
  BufNeed need;
};

// 1. The refusals, the previous launch's sticky error, the pass and launch plans, the kernel.
int plan_frame(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles, void* hip_stream,
               bool run_pass, uint32_t n_samples, Frame* f) {
  if (!c || !cam || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  int rc = plan_pass(p, run_pass ? c->run.done : 0u, run_pass ? n_samples : (p ? p->samples_per_pixel : 0u), &f->pass);
  if (rc) return rc;
  rc = params_fit_ctx(c, p);
  if (rc) return rc;
  HIPCHK(hipSetDevice(c->device));
  // a device error of the previous launch that finished meanwhile is reported
  // here (sticky), so a caller that never synchronises through the ABI still sees it
  rc = launch_status(c, false);
  if (rc) return rc;
  f->cam = cam;
  f->p = p;
  f->dev_tiles = dev_tiles;
  f->st = stream_of(c, hip_stream);
  f->run_pass = run_pass;
  f->first = !run_pass || c->run.passes == 0;
  f->adapt = run_pass && c->adapt.on;
  f->diag = (p->flags & ZRT_FLAG_STATS) != 0;
  f->g = geometry(p);
  f->my_tiles = rank_tiles(f->g, p->rank, p->world_size);
  f->plan = plan_launch(c->scene.shape, p);
  f->cam_inside = camera_inside(cam, c->scene.root_c, c->scene.origin_bound);
  f->kfn = select_kernel(f->plan.kmode, p->prng, f->diag, f->plan.stk16, lean_launch(f->plan, f->diag, f->cam_inside));
  return ZRT_OK;
}

// 2. Occupancy gives the grid; the grid gives the lanes, the paths and the global rows.
int size_frame(const zrt_ctx* c, const Frame& f, FrameSize* z) {
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&z->per_cu, f.kfn, kBlock, f.plan.lp.bytes));
  z->per_cu = std::max(1, std::min(z->per_cu, 8));
  z->n_act = f.adapt ? c->adapt.n_active : f.my_tiles;
  z->work = uint32_t(uint64_t(z->n_act) * f.pass.pass_chunks);
  // one wave per unit at the start; more waves than units would only idle
  z->grid = std::max(1u, std::min(uint32_t(c->cu_count) * uint32_t(z->per_cu), (z->work + (kBlock / 64) - 1) / (kBlock / 64)));
  z->n_lanes = uint64_t(z->grid) * kBlock;
  // global attenuation rows: [row][lane], or [path][row] for the path-pool loop
  z->n_paths = f.plan.pool ? uint64_t(z->grid) * K.block_paths : z->n_lanes;
  if (z->n_paths >= (1ull << 32)) return fail(ZRT_E_UNSUPPORTED, "too many paths");
  z->need = buffer_need(f.plan.lp, f.p->max_depth, f.plan.stack_depth, z->n_paths, z->n_lanes, f.plan.stk16);
  if (z->need.att_elems * sizeof(uint32_t) > (16ull << 30))
    return fail(ZRT_E_UNSUPPORTED, "max_depth too large for the per-lane attenuation stack");
  return ZRT_OK;
}

// 3. The buffers grown to the launch's need, and what it adds into zeroed.
void prepare_buffers(zrt_ctx* c, const Frame& f, const FrameSize& z) {
  c->partial.grow(uint64_t(f.my_tiles) * 64u * f.pass.pass_chunks);
  c->att.grow(z.need.att_elems);
  if (z.need.ovf_bytes) c->stack_ovf.grow(z.need.ovf_bytes);
  if (f.first)
    HIPCHK(hipMemsetAsync(c->scratch.p, 0, kScratchSlots * sizeof(unsigned long long), f.st));
  else  // a run's later passes add into its counters and keep its error flag: a new work counter only
    HIPCHK(hipMemsetAsync(c->scratch.p + kWorkSlot, 0, sizeof(unsigned long long), f.st));
  if (f.run_pass && f.first) {
    HIPCHK(hipMemsetAsync(c->run.accum.p, 0, c->run.accum.n * sizeof(float4), f.st));
    if (f.adapt) HIPCHK(hipMemsetAsync(c->adapt.tile_done.p, 0, c->adapt.tile_done.n * sizeof(uint32_t), f.st));
  }
}

// 4. A run's later pass: the previous pass's events wait to be added into the run's
// times (no host wait here), and the pass takes a spare set.
void rotate_events(zrt_ctx* c) {
  AccumRun& r = c->run;
  fold_pass_times(c, false);  // (frees the sets of passes that have finished)
  if (r.spare.empty()) {
    r.spare.emplace_back();
    r.spare.back().create();
  }
  r.pending.push_back(std::move(c->ev));
  c->ev = std::move(r.spare.back());
  r.spare.pop_back();
}

// 5. The kernel's arguments, but for the tile order and the optional outputs.
KArgs fill_args(const zrt_ctx* c, const Frame& f, const FrameSize& z, const LaunchEnv& env) {
  const LaunchPlan& P = f.plan;
  KArgs a{};
  fill_scene(a, c, P.qn, P.stack_depth);
  fill_camera(a, f.cam, f.p);
  fill_lds(a, P.lp);
  a.att = c->att.p;
  a.partial = c->partial.p;
  a.counters = c->scratch.p;
  a.work_counter = reinterpret_cast<uint32_t*>(c->scratch.p + kWorkSlot);
  a.color_scale = 1.0f / float(f.pass.samples_after);  // raytrace.zig:157
  a.spp = f.pass.pass_samples;
  a.max_depth = f.p->max_depth;
  a.tiles_x = f.g.tiles_x;
  a.rank = f.p->rank;
  a.world = f.p->world_size;
  a.total_work = z.work;
  a.guard = P.guard_on ? c->scene.shape.guard : 0.0f;
  a.check_origins = f.cam_inside ? 0u : 1u;
  if (z.need.ovf_bytes) a.stack_ovf = c->stack_ovf.p;
  a.n_lanes = uint32_t(z.n_lanes);
  a.n_paths = uint32_t(z.n_paths);
  // (a loop that reads the table from LDS only and has none there - the lockstep loop
  // at max_depth 0, which shades nothing - copies none: its plan holds no region for it)
  if (P.kmode == 3 && !P.lp.mats_in_lds) a.n_mats = 0u;
  a.seed_mix = f.p->seed * 0x9E3779B97F4A7C15ULL + f.pass.key_offset;
  a.chunk = f.pass.chunk;
  a.n_chunks = f.pass.pass_chunks;
  a.wf_thresh = env.wf_thresh;
  // the lockstep interval: the BVH loops keep a wave's lanes on one sample (its
  // camera rays coherent); the list loop gains nothing from that (every ray reads
  // the same surfaces) and lets its lanes run through the unit's chunk
  // (C2: 34.1 -> 45.4 Gray/s, profiles/r04/s1)
  a.sync = env.sync ? env.sync : P.mode == 0 ? f.pass.chunk : K.sync_samples;
  a.n_slots = f.my_tiles * 64u;
  if (env.debug)
    std::fprintf(stderr, "zrt launch: mode %d stk16 %d grid %u (%d blocks/CU x %d CUs) lds %zu B "
                 "(stack rows %u, top nodes %u @%u, att rows %u @%u, mats %u @%u)\n", P.mode, int(P.stk16), z.grid,
                 z.per_cu, c->cu_count, P.lp.bytes, P.lp.stack_rows, a.n_top, P.lp.top_off, P.lp.att_rows, P.lp.att_off,
                 P.lp.mats_in_lds ? c->scene.shape.n_mats : 0u, P.lp.mat_off);
  return a;
}

// 6. The order the launch hands its tiles out in: a run's later pass reuses its first
// pass's; a frame takes the order kept under its key, else probes (schedule_tiles);
// an adaptive level hands out its active list.  Returns whether the launch is scheduled.
bool choose_order(zrt_ctx* c, const Frame& f, const FrameSize& z, const LaunchEnv& env, KArgs& a) {
  const zrt_params* p = f.p;
  Probe& pr = c->probe;
  HIPCHK(hipEventRecord(c->ev.pre, f.st));
  bool schedule =
      f.plan.mode == 3 && !(p->flags & ZRT_FLAG_NO_SCHEDULE) && p->samples_per_pixel >= 128 && f.my_tiles >= 2;
  // (a run decides once, by its cap: its first pass probes, the later ones reuse the
  // order and the probe's counters)
  bool order_hit = false;  // the context holds the order of a probe with this launch's key
  if (schedule && !f.first) {
    schedule = c->run.ordered;
    if (schedule) a.tile_order = pr.tile_order.p;
  } else if (schedule) {
    // (the order cannot change a frame - chunk sums land in fixed slots - so a frame
    // with another seed, sample count or PRNG takes it too)
    const OrderKey key{*f.cam, p->width, p->height, p->max_depth, p->rank, p->world_size, p->traversal,
                       f.plan.guard_on ? 1u : 0u, f.my_tiles};
    order_hit = env.order_cache && pr.order_valid && std::memcmp(&key, &pr.order_key, sizeof(key)) == 0;
    if (order_hit) {
      a.tile_order = pr.tile_order.p;
    } else {
      pr.order_valid = false;  // (the probe overwrites the order, whether or not it completes)
      schedule = schedule_tiles(c, a, p->prng, f.plan.stk16, f.my_tiles, z.grid, f.st);
      pr.order_key = key;
      pr.order_valid = schedule;
    }
  }
  if (f.run_pass && f.first) c->run.ordered = schedule;
  if (f.adapt) {
    // the launch hands out the active list: level 0's is the probe's order where the run
    // is scheduled (else the identity zrt_ctx_adapt_begin uploaded), a later level's is
    // what the previous level's compaction wrote
    uint32_t* list = c->adapt.active[c->adapt.cur].p;
    if (f.first && schedule)
      HIPCHK(hipMemcpyAsync(list, pr.tile_order.p, size_t(f.my_tiles) * sizeof(uint32_t), hipMemcpyDeviceToDevice, f.st));
    a.tile_order = list;
  }
  c->ev.probed = schedule && f.first && !order_hit;
  return schedule;
}

// 6b. The all-sky tiles split off (tile_class.cpp proves them; sky_kernel renders them
// without traversal): the render launch keeps the general tiles, in the order chosen
// above, and its work shrinks to match.  The classes and the lists are kept under the
// order cache's key: a frame with a matching key classifies nothing, and a run's later
// pass takes its first pass's.  Classification runs here, behind the enqueued probe and
// before e0, so a scheduled launch's schedule_ms covers it.  An adaptive level does not
// take the split (its active list changes from level to level on the device).
// The one-sphere tiles (their camera rays can hit one sphere alone: the ONE_SPHERE
// kernels test it without walking the tree) are split off the same way, into a third
// list in the same order, where sphere_split_allowed and ZRT_SPHERE_TILES say so.
// Returns the sky and one-sphere tiles (0, 0: no split; a.tile_order and a.total_work are
// as they were) and where the one-sphere launch reads its list.
struct TileSplit {
  uint32_t n_sky = 0, n_one = 0;
  const uint32_t* one_order = nullptr;
};
TileSplit split_sky(zrt_ctx* c, const Frame& f, const LaunchEnv& env, KArgs& a) {
  const zrt_params* p = f.p;
  SkySplit& sp = c->sky;
  if (!env.sky_tiles || f.adapt || f.my_tiles == 0 || !sp.scene.ok || !sky_split_allowed(f.plan, p, f.cam_inside))
    return {};
  const bool want_one = env.sphere_tiles && sphere_split_allowed(f.plan, p, f.cam_inside);
  const OrderKey key{*f.cam, p->width, p->height, p->max_depth, p->rank, p->world_size, p->traversal,
                     f.plan.guard_on ? 1u : 0u, f.my_tiles};
  const bool hit = sp.valid && std::memcmp(&key, &sp.key, sizeof(key)) == 0 && sp.key_sphere == want_one &&
                   (env.order_cache || !f.first);
  if (!hit) {
    sp.valid = false;
    const double t0 = now_ms();
    OneSphere one;
    one.want = want_one;
    classify_tiles(sp.scene, f.cam, p, &sp.cls, &sp.n_sky, nullptr, &one);
    sp.n_one = one.n_tiles;
    sp.one_sphere = one.sphere;
    if (env.debug)
      std::fprintf(stderr, "zrt launch: %u of %u tiles all sky, %u one-sphere, classified in %.2f ms\n", sp.n_sky,
                   f.my_tiles, sp.n_one, now_ms() - t0);
    sp.sky_host.clear();
    sp.gen_host.clear();
    sp.one_host.clear();
    for (uint32_t lt = 0; lt < f.my_tiles; ++lt)
      (sp.cls[lt] == kTileSky ? sp.sky_host : sp.cls[lt] == kTileGeneral ? sp.gen_host : sp.one_host).push_back(lt);
    if (sp.n_sky || sp.n_one) {
      // (stream-ordered behind the previous launch, which may still read the old lists)
      if (sp.cls_dev.n < f.my_tiles) {
        HIPCHK(hipStreamSynchronize(f.st));
        sp.cls_dev.alloc(f.my_tiles);
        sp.sky_list.alloc(f.my_tiles);
        sp.gen_list.alloc(f.my_tiles);
        sp.one_list.alloc(f.my_tiles);
        sp.gen_sorted.alloc(f.my_tiles);
        sp.one_sorted.alloc(f.my_tiles);
        sp.count.alloc(1);
      }
      const auto up = [&](DevBuf<uint32_t>& d, const std::vector<uint32_t>& h) {
        if (!h.empty()) HIPCHK(hipMemcpyAsync(d.p, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice, f.st));
      };
      up(sp.cls_dev, sp.cls);
      up(sp.sky_list, sp.sky_host);
      up(sp.gen_list, sp.gen_host);
      up(sp.one_list, sp.one_host);
      HIPCHK(hipStreamSynchronize(f.st));  // (the host vectors are rewritten by the next classification)
    }
    sp.sorted_valid = false;
    sp.key = key;
    sp.key_sphere = want_one;
    sp.valid = true;
  }
  if (sp.n_sky == 0 && sp.n_one == 0) return {};
  TileSplit ts;
  ts.n_sky = sp.n_sky;
  ts.n_one = sp.n_one;
  const uint32_t n_gen = f.my_tiles - sp.n_sky - sp.n_one;
  if (a.tile_order) {  // the probe's cost order, each class's tiles of it
    if (!sp.sorted_valid || sp.sorted_gen != c->probe.order_gen) {
      if (sp.n_one) {
        HIPCHK(launch_compact_class(f.st, c->probe.tile_order.p, f.my_tiles, sp.cls_dev.p, kTileGeneral, sp.gen_sorted.p,
                                    sp.count.p));
        HIPCHK(launch_compact_class(f.st, c->probe.tile_order.p, f.my_tiles, sp.cls_dev.p, sp.cls[sp.one_host[0]],
                                    sp.one_sorted.p, sp.count.p));
      } else {
        HIPCHK(launch_compact(f.st, c->probe.tile_order.p, f.my_tiles, sp.cls_dev.p, sp.gen_sorted.p, sp.count.p));
      }
      sp.sorted_gen = c->probe.order_gen;
      sp.sorted_valid = true;
    }
    a.tile_order = sp.gen_sorted.p;
    ts.one_order = sp.one_sorted.p;
  } else {
    a.tile_order = sp.gen_list.p;
    ts.one_order = sp.one_list.p;
  }
  a.total_work = uint32_t(uint64_t(n_gen) * f.pass.pass_chunks);
  return ts;
}

// 7. The lockstep interval's probe, the scanline and wave-time outputs, and - the
// probe may have grown them - the global rows' buffers and their bounds.
void optional_outputs(zrt_ctx* c, const Frame& f, const FrameSize& z, const LaunchEnv& env, bool schedule, KArgs& a) {
  // the lockstep loop takes its interval from the probe's lane efficiency (auto_sync)
  a.sync_probe = schedule && f.plan.kmode == 3 && env.auto_sync ? c->probe.scratch.p : nullptr;
  if (f.p->flags & ZRT_FLAG_SCANLINES) {  // (not the probe's: set after it)
    const size_t n = size_t(f.p->height) * 3;
    c->scanlines.grow(n);
    if (f.first) HIPCHK(hipMemsetAsync(c->scanlines.p, 0, n * sizeof(unsigned long long), f.st));
    a.scanlines = c->scanlines.p;
  }
  if (K.profile) {
    c->wave_times.grow(2ull * z.grid * (kBlock / 64));
    a.wave_times = c->wave_times.p;
  }
  // every global row the render launch may touch lies inside its buffer: checked on
  // the host, and handed to the STATS flavour's device check
  check_buffers("render launch", z.need, c->att.n, c->stack_ovf.n);
  a.att = c->att.p;
  if (z.need.ovf_bytes) a.stack_ovf = c->stack_ovf.p;
  a.att_cap = c->att.n;
  a.ovf_cap = ovf_cap_elems(c->stack_ovf.n, f.plan.stk16);
  if (f.diag && env.cap_rows) {
    a.att_cap = uint64_t(double(a.att_cap) * env.row_cap);
    a.ovf_cap = uint64_t(double(a.ovf_cap) * env.row_cap);
  }
}

// 8. The kernel between its events, and what resolves its chunk sums into dev_tiles:
// finalize (a frame), accumulate (a pass), or resolve and compact (an adaptive level).
void enqueue(zrt_ctx* c, const Frame& f, const FrameSize& z, const LaunchEnv& env, KArgs& a, const TileSplit& ts) {
  const uint32_t n_sky = ts.n_sky;
  const zrt_params* p = f.p;
  const Geometry& g = f.g;
  const uint32_t n_chunks = f.pass.pass_chunks, n_slots = f.my_tiles * 64u;
  unsigned long long* err = c->scratch.p + kErrorSlot;
  HIPCHK(hipEventRecord(c->ev.e0, f.st));
  if (n_sky > 0) {  // the all-sky tiles: one wave per unit at the most, no LDS
    KArgs sa = a;
    sa.tile_order = c->sky.sky_list.p;
    sa.total_work = uint32_t(uint64_t(n_sky) * n_chunks);
    const uint32_t grid = std::max(1u, std::min(uint32_t(c->cu_count) * 8u, (sa.total_work + kBlock / 64 - 1) / (kBlock / 64)));
    void* args[] = {&sa};
    if (env.sky_by_render) {  // (what the sky tiles cost in the render kernel: its own launch, its own work counter)
      HIPCHK(hipLaunchKernel(f.kfn, dim3(z.grid), dim3(kBlock), args, f.plan.lp.bytes, f.st));
      HIPCHK(hipMemsetAsync(c->scratch.p + kWorkSlot, 0, sizeof(unsigned long long), f.st));
    } else {
      HIPCHK(hipLaunchKernel(sky_kernel_ptr(p->prng, f.diag), dim3(grid), dim3(kBlock), args, 0, f.st));
    }
  }
  if (ts.n_one > 0) {  // the one-sphere tiles: the same loop, its camera rays' step without the tree
    const SkySplit& sp = c->sky;
    KArgs oa = a;
    oa.tile_order = ts.one_order;
    oa.total_work = uint32_t(uint64_t(ts.n_one) * n_chunks);
    const SphereArgs& sa = sp.scene.sphere_args[size_t(sp.one_sphere)];
    std::memcpy(oa.one_lo, sa.lo, sizeof(sa.lo));
    std::memcpy(oa.one_hi, sa.hi, sizeof(sa.hi));
    std::memcpy(oa.one_rec, sa.rec, sizeof(sa.rec));
    oa.one_slot = sp.scene.spheres[size_t(sp.one_sphere)];
    // (ZRT_SPHERE_TILES=2: what these tiles cost in the render kernel)
    void* kfn = env.sphere_by_render ? f.kfn : one_sphere_kernel(p->prng, f.diag, f.plan.stk16);
    const uint32_t grid = std::max(1u, std::min(z.grid, (oa.total_work + kBlock / 64 - 1) / (kBlock / 64)));
    void* args[] = {&oa};
    HIPCHK(hipLaunchKernel(kfn, dim3(grid), dim3(kBlock), args, f.plan.lp.bytes, f.st));
    HIPCHK(hipMemsetAsync(c->scratch.p + kWorkSlot, 0, sizeof(unsigned long long), f.st));  // its own work counter
  }
  if (a.total_work > 0) {
    void* args[] = {&a};
    HIPCHK(hipLaunchKernel(f.kfn, dim3(z.grid), dim3(kBlock), args, f.plan.lp.bytes, f.st));
  }
  HIPCHK(hipEventRecord(c->ev.e1, f.st));
  if (!f.run_pass) {
    if (f.my_tiles > 0)
      HIPCHK(launch_finalize(f.st, c->partial.p, f.dev_tiles, n_slots, n_chunks, p->world_size, p->rank, g.tiles_x,
                             g.xbound, p->height, a.color_scale, err));
    return;
  }
  AccumRun& r = c->run;
  HIPCHK(hipMemsetAsync(r.metrics.p, 0, kMetricWords * sizeof(unsigned long long), f.st));
  // the chunk sums that enter the second moment: all but a ragged last one (zrt.h "the variance plane")
  const uint32_t q_chunks = n_chunks - (f.pass.last_chunk < f.pass.chunk ? 1u : 0u);
  const float prev_scale = r.done ? 1.0f / float(r.done) : 0.0f;
  if (f.adapt) {
    // resolve the active tiles, decide (levels 1 .. last - 1), pack the survivors in
    // order into the other list; the host reads their number (zrt_ctx_adapt_level)
    AdaptRun& ad = c->adapt;
    const uint32_t decide = ad.k >= 1 && ad.k + 1 < ad.levels.size() ? 1u : 0u;
    HIPCHK(hipMemsetAsync(ad.active_count.p, 0, sizeof(uint32_t), f.st));
    if (z.n_act > 0) {
      HIPCHK(launch_resolve(f.st, c->partial.p, r.accum.p, f.dev_tiles, ad.active[ad.cur].p, z.n_act, f.my_tiles,
                            n_chunks, p->world_size, p->rank, g.tiles_x, g.xbound, p->height, prev_scale, a.color_scale,
                            q_chunks, ad.a.tolerance, decide, f.pass.samples_after, ad.tile_done.p, err, r.metrics.p));
      HIPCHK(launch_compact(f.st, ad.active[ad.cur].p, z.n_act, ad.tile_done.p, ad.active[ad.cur ^ 1u].p,
                            ad.active_count.p));
    }
    HIPCHK(hipMemcpyAsync(ad.count_host.get(), ad.active_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, f.st));
  } else if (f.my_tiles > 0) {
    HIPCHK(launch_accumulate(f.st, c->partial.p, r.accum.p, f.dev_tiles, n_slots, n_chunks, p->world_size, p->rank,
                             g.tiles_x, g.xbound, p->height, prev_scale, a.color_scale, q_chunks, err, r.metrics.p));
  }
  HIPCHK(hipMemcpyAsync(r.metrics_host.get(), r.metrics.p, kMetricWords * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        f.st));
}

// 9. The error flag copied back behind the done event; the launch recorded; the run advanced.
void finish(zrt_ctx* c, const Frame& f, const FrameSize& z, const KArgs& a, bool schedule, const TileSplit& ts) {
  HIPCHK(hipMemcpyAsync(c->render.err.get(), c->scratch.p + kErrorSlot, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        f.st));
  HIPCHK(hipEventRecord(c->render.done, f.st));
  c->render.launched = true;
  c->render.reported = false;
  LastLaunch l;
  l.g = f.g;
  l.height = f.p->height;
  l.rank = f.p->rank;
  l.world = f.p->world_size;
  l.tiles = f.my_tiles;
  uint64_t pixels = 0;  // the pixels this rank renders (for the samples / pixels counters)
  for_rank_tiles(f.g, l.height, l.rank, l.world,
                 [&pixels](uint32_t, uint32_t w, uint32_t h, uint32_t) { pixels += uint64_t(w) * h; });
  l.pixels = uint32_t(pixels);
  l.spp = f.pass.samples_after;
  l.stats = f.diag;
  l.qn = f.plan.qn;
  l.run = f.run_pass;
  l.adapt = f.adapt;
  l.scheduled = schedule;
  l.mode = f.plan.mode;
  l.loop = int(reported_loop(f.plan.kmode));
  l.guard = a.guard;
  l.scanline_rows = (f.p->flags & ZRT_FLAG_SCANLINES) ? f.p->height : 0u;
  l.n_waves = K.profile ? z.grid * (kBlock / 64) : 0u;
  l.sky_tiles = ts.n_sky;
  l.sphere_tiles = ts.n_one;
  c->last = l;
  if (f.run_pass) {
    c->run.done = f.pass.samples_after;
    c->run.passes += 1;
    c->run.pass_samples = f.pass.pass_samples;
  } else {
    c->run.live = false;  // a plain render overwrites the probe's buffers: it ends the run
  }
}
}  // namespace

// The launch behind zrt_ctx_render_tiles (run_pass false: the whole frame) and
// zrt_ctx_accum_pass / zrt_ctx_adapt_level (run_pass true: samples [run.done, run.done +
// n_samples) of the context's run, p = its params): one launch path and one kernel
// choice for all three.
int launch_frame(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles, void* hip_stream,
                 bool run_pass, uint32_t n_samples) {
  try {
    Frame f{};
    int rc = plan_frame(c, cam, p, dev_tiles, hip_stream, run_pass, n_samples, &f);
    if (rc) return rc;
    FrameSize z{};
    rc = size_frame(c, f, &z);
    if (rc) return rc;
    const LaunchEnv env = read_launch_env();
    prepare_buffers(c, f, z);
    if (run_pass && !f.first) rotate_events(c);
    KArgs a = fill_args(c, f, z, env);
    const bool schedule = choose_order(c, f, z, env, a);
    const TileSplit ts = split_sky(c, f, env, a);
    optional_outputs(c, f, z, env, schedule, a);
    enqueue(c, f, z, env, a, ts);
    finish(c, f, z, a, schedule, ts);
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}
}  // namespace zrt

using zrt::fail;

int zrt_abi_version(void) { return ZRT_ABI_VERSION; }

const char* zrt_build_info(void) {
  return "libzrt: HIP path for gfx950 (MI355X); persistent wave64 path-tracing kernel; -ffp-contract=off";
}

int zrt_ctx_create(const zrt_scene* scene, const zrt_params* params, zrt_ctx** out) {
  if (!out) return fail(ZRT_E_INVALID, "out is null");
  *out = nullptr;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (!params) return fail(ZRT_E_INVALID, "params is null");
  try {
    // raytrace.zig:124-133: BVH iff requested and more than 10 surfaces.  The
    // scene is flattened before the device is checked, so a tree whose layout
    // the kernels do not decode is refused on any machine (flatten_scene); the
    // GPU builds the reference BVH only when one is visible
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;
    int n_dev = 0;
    const bool gpus = hipGetDeviceCount(&n_dev) == hipSuccess && n_dev > 0;
    // with GPUs present, an unusable device is refused before the (seconds-long on a
    // million-triangle mesh) scene build; without any, the layout check still runs first
    if (gpus) {
      rc = zrt::check_device(int(params->device));
      if (rc) return rc;
    }
    const bool have_dev = gpus && int(params->device) < n_dev;
    zrt::HostScene h;
    zrt::flatten_for_device(&h, scene, use_bvh, have_dev ? int(params->device) : -1);
    rc = zrt::check_device(int(params->device));
    if (rc) return rc;
    *out = zrt::ctx_on_device(h, int(params->device)).release();
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_destroy(zrt_ctx* ctx) {
  if (!ctx) return ZRT_OK;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;
  return ZRT_OK;
}

int zrt_ctx_tile_count(const zrt_ctx* ctx, const zrt_params* params, uint32_t* n_tiles) {
  (void)ctx;  // the partition depends on the params only; ctx may be NULL
  if (!n_tiles) return fail(ZRT_E_INVALID, "null argument");
  const int rc = zrt::validate_params(params);
  if (rc) return rc;
  *n_tiles = zrt::rank_tiles(zrt::geometry(params), params->rank, params->world_size);
  return ZRT_OK;
}

int zrt_ctx_render_tiles(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles,
                         void* hip_stream) {
  return zrt::launch_frame(c, cam, p, dev_tiles, hip_stream, false, 0);
}

int zrt_ctx_stats(zrt_ctx* c, zrt_stats* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->render.launched) return fail(ZRT_E_INVALID, "zrt_ctx_stats before any zrt_ctx_render_tiles");
  try {
    const zrt::Scene& s = c->scene;
    const zrt::LastLaunch& l = c->last;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->render.done));
    unsigned long long h[zrt::kScratchSlots] = {0};
    HIPCHK(hipMemcpy(h, c->scratch.p, sizeof(h), hipMemcpyDeviceToHost));
    if (l.scanline_rows) {  // ZRT_FLAG_SCANLINES: the launch counted these three per row only
      std::vector<unsigned long long> rows(size_t(l.scanline_rows) * 3);
      HIPCHK(hipMemcpy(rows.data(), c->scanlines.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      for (size_t y = 0; y < l.scanline_rows; ++y) {
        h[zrt::kDepthHits] += rows[3 * y];
        h[zrt::kReflections] += rows[3 * y + 1];
        h[zrt::kBackground] += rows[3 * y + 2];
      }
    }
    std::memset(out, 0, sizeof(*out));
    out->recursion_depth_hits = h[zrt::kDepthHits];
    out->reflections = h[zrt::kReflections];
    out->background_hits = h[zrt::kBackground];
    // rayColor calls = samples + reflections = rays + depth-limit hits
    // (an adaptive run: per-tile sample counts, summed level by level)
    const uint64_t samples = l.adapt ? c->adapt.samples : uint64_t(l.pixels) * l.spp;
    out->rays_processed = l.stats ? h[zrt::kRays] : samples + h[zrt::kReflections] - h[zrt::kDepthHits];
    out->node_visits = h[zrt::kNodes];
    out->prim_tests = h[zrt::kTriTests] + h[zrt::kSphereTests];
    out->sphere_tests = h[zrt::kSphereTests];
    out->shade_fetches = h[zrt::kShades];
    out->texel_fetches = h[zrt::kTexels];
    out->leaf_visits = h[zrt::kLeaves];
    out->order_replays = h[zrt::kReplays];
    uint32_t bt = uint32_t(h[zrt::kExcessTri]), bs = uint32_t(h[zrt::kExcessSph]);
    std::memcpy(&out->box_excess_max_triangle, &bt, 4);
    std::memcpy(&out->box_excess_max_sphere, &bs, 4);
    out->box_excess_hits = h[zrt::kExcessHits];
    // FAST: leaf boxes ride in their parent's 128 B; compressed: 64-B nodes (+ 32-B leaf records)
    out->node_bytes = l.mode == 3 ? (l.qn ? 64 : 128) : 32;
    out->wide_nodes = s.shape.n_wide;
    out->sampling_loop = uint32_t(l.loop);
    out->guard = l.guard;
    out->texel_bytes = s.texel_bytes;
    out->pixels_processed = l.pixels;
    out->samples_processed = samples;
    out->preprocess_ms = s.preprocess_ms;
    out->upload_ms = s.upload_ms;
    const zrt::LaunchTimes t = zrt::launch_times(c->ev);
    out->render_ms = t.render_ms;
    out->schedule_ms = t.schedule_ms;
    if (l.run) {  // a run: the sums over its passes (the counters above were never re-zeroed)
      zrt::fold_pass_times(c, true);
      out->render_ms = c->run.render_ms + t.render_ms;
      out->schedule_ms = float(c->run.sched_ms + t.schedule_ms);
    }
    out->used_bvh = s.shape.use_bvh ? 1 : 0;
    out->bvh_nodes = s.shape.n_nodes;
    out->bvh_max_depth = s.bvh_depth;
    out->n_gpus = 1;
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_sync(zrt_ctx* c) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  try {
    HIPCHK(hipSetDevice(c->device));
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_last_kernel_ms(zrt_ctx* c, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!c->render.launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev.e1));
    *ms = zrt::launch_times(c->ev).kernel_ms;
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

namespace zrt {
// The per-row Progress counters of c's last launch (ZRT_FLAG_SCANLINES) added
// into out[0 .. height): this rank's pixels, samples and rays of each row and
// the three counters the kernel counted per row.
int add_scanlines(zrt_ctx* c, zrt_scanline* out, uint32_t height) {
  const LastLaunch& l = c->last;
  if (!c->render.launched || l.scanline_rows == 0)
    return fail(ZRT_E_INVALID, "the last launch did not count scanlines (ZRT_FLAG_SCANLINES)");
  if (height != l.scanline_rows) return fail(ZRT_E_INVALID, "height differs from the last launch's");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->render.done));
  std::vector<unsigned long long> rows(size_t(height) * 3);
  HIPCHK(hipMemcpy(rows.data(), c->scanlines.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<uint32_t> done;  // an adaptive run: samples per pixel of each tile
  if (l.adapt) {
    done.resize(std::max(1u, l.tiles));
    HIPCHK(hipMemcpy(done.data(), c->adapt.tile_done.p, size_t(l.tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  std::vector<uint64_t> row_samples(height, 0);
  // pixels of this rank's tiles, per row
  for_rank_tiles(l.g, height, l.rank, l.world, [&](uint32_t lt, uint32_t w, uint32_t h, uint32_t y0) {
    const uint32_t spp = l.adapt ? done[lt] & ~kTileFrozen : l.spp;
    for (uint32_t y = y0; y < y0 + h; ++y) {
      out[y].pixels += w;
      row_samples[y] += uint64_t(w) * spp;
    }
  });
  for (uint32_t y = 0; y < height; ++y) {
    out[y].recursion_depth_hits += rows[3 * y];
    out[y].reflections += rows[3 * y + 1];
    out[y].background_hits += rows[3 * y + 2];
  }
  // samples and rays from the pixels (rays = rayColor calls - depth-limit hits)
  for (uint32_t y = 0; y < height; ++y) {
    out[y].samples += row_samples[y];
    out[y].rays = out[y].samples + out[y].reflections - out[y].recursion_depth_hits;
  }
  return ZRT_OK;
}
}  // namespace zrt

int zrt_ctx_scanlines(zrt_ctx* c, zrt_scanline* out, uint32_t height) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  try {
    std::memset(out, 0, sizeof(zrt_scanline) * height);
    int rc = zrt::add_scanlines(c, out, height);
    if (rc) return rc;
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_assemble(zrt_ctx* c, const zrt_params* p, const float* dev_gathered, float* dev_frame,
                     void* hip_stream) {
  return zrt::assemble(c, p, dev_gathered, 0, dev_frame, hip_stream);
}

int zrt_ctx_assemble_padded(zrt_ctx* c, const zrt_params* p, const float* dev_gathered, uint32_t stride_tiles,
                            float* dev_frame, void* hip_stream) {
  if (stride_tiles == 0) return fail(ZRT_E_INVALID, "stride_tiles must be > 0");
  return zrt::assemble(c, p, dev_gathered, stride_tiles, dev_frame, hip_stream);
}

int zrt_ctx_assemble_plane(zrt_ctx* c, const zrt_params* p, const float* dev_gathered, uint32_t stride_tiles,
                           float* dev_frame, void* hip_stream) {
  return zrt::assemble(c, p, dev_gathered, stride_tiles, dev_frame, hip_stream, 1);
}
