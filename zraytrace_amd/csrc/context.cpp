// context.cpp - the device-resident scene behind zrt_ctx_*: upload, the frame
// launch (render, accumulation pass, adaptive level) with its scheduling probe,
// the first-hit features, the denoise and assemble calls, zrt_trace and the
// debug entry points that run a kernel.  The kernels themselves: render.hip.
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
static void upload_scene(zrt_ctx* c, const HostScene& h) {
  const double t1 = now_ms();
  c->nodes.upload(h.nodes);
  c->wnodes.upload(h.wn);
  if (h.q_ok) {
    c->qnodes.upload(h.qn);
    c->qleaves.upload(h.ql);
  }
  c->q_ok = h.q_ok;
  c->q_stride = h.q_stride;
  c->q_top = h.q_top;
  c->n_qleaves = uint32_t(h.ql.size() / kLeafRecF4);
  c->prims.upload(h.prims);
  c->shade.upload(h.shade);
  c->mats.upload(h.mats);
  c->texels.upload(h.tex);
  c->texels8.upload(h.tex8);
  c->leaf_of_slot.upload(h.leaf_of_slot);
  c->ref_sph.upload(h.ref_sph);
  for (int k = 0; k < 3; ++k) c->root_c[k] = h.root_c[k];
  c->origin_bound = h.origin_bound;
  c->layout = h.layout;
  c->graze_m = h.graze_m;
  c->graze_leaf = h.graze_leaf;
  c->guard = h.guard;
  c->upload_ms = now_ms() - t1;
  c->preprocess_ms = h.preprocess_ms;
  c->use_bvh = h.use_bvh;
  c->n_prims = h.n_prims;
  c->n_nodes = h.n_nodes;
  c->bvh_depth = h.bvh_depth;
  c->stack_depth = h.use_bvh ? h.bvh_depth + 2 : 0;
  c->n_wide = h.n_wide;
  c->n_leaves = h.n_leaves;
  c->n_top = h.n_top;
  c->n_mats = uint32_t(h.mats.size());
  c->wide_stack = h.wide_stack;
  c->wide_stride = h.wide_stride;
  c->texel_bytes = h.texel_bytes;
  c->tri_rcp_fast = h.tri_rcp_fast;
  c->scene_extent = h.scene_extent;
  for (int k = 0; k < 3; ++k) {
    c->tri_c[k] = h.tri_c[k];
    c->tri_h[k] = h.tri_h[k];
  }
  c->slot_to_prim = h.slot_to_prim;
  c->shape = shape_of(h);
}

// ---- KArgs, filled once (kernels.hpp): each launch adds only what is its own ----
// The tree a launch traverses: the full wide nodes, or (qn) the compressed ones.
static void fill_tree(KArgs& a, const zrt_ctx* c, bool qn) {
  a.wnodes = qn ? c->qnodes.p : c->wnodes.p;
  a.wide_stride = qn ? c->q_stride : c->wide_stride;
  a.node_f4 = qn ? kQuantNodeF4 : 8u;
  a.qleaves = qn ? c->qleaves.p : nullptr;
  a.n_qnodes = qn ? c->q_stride / kQuantNodeF4 : 0u;
  a.n_qleaves = qn ? c->n_qleaves : 0u;
  a.n_top = qn ? c->q_top : c->n_top;
}
// The scene part: the context's buffers and constants, its error flag, and the
// traversal stack's depth (the reference traversal's rows: at most its own).
static void fill_scene(KArgs& a, const zrt_ctx* c, bool qn, uint32_t stack_depth) {
  a.nodes = c->nodes.p;
  a.prims = c->prims.p;
  a.shade = c->shade.p;
  a.mats = c->mats.p;
  a.texels = c->texels.p;
  a.texels8 = c->texels8.p;
  a.n_mats = c->n_mats;
  fill_tree(a, c, qn);
  a.error_flag = reinterpret_cast<uint32_t*>(c->scratch.p + kErrorSlot);
  a.n_list = c->use_bvh ? 0 : c->n_prims;
  a.tri_rcp_fast = c->tri_rcp_fast;
  a.scene_extent = c->scene_extent;
  a.paxis_m = paxis_threshold();
  for (int k = 0; k < 3; ++k) {
    a.tri_c[k] = c->tri_c[k];
    a.tri_h[k] = c->tri_h[k];
    a.root_c[k] = c->root_c[k];
  }
  a.stack_depth = stack_depth;
  a.ref_stack = std::min(c->stack_depth, stack_depth);
  a.leaf_of_slot = c->leaf_of_slot.p;
  a.ref_sph = c->ref_sph.p;
  a.origin_bound = c->origin_bound;
  a.layout = c->layout;
  a.graze_m = c->graze_m;
  a.graze_leaf = c->graze_leaf;
}
// The camera and the frame's size.
static void fill_camera(KArgs& a, const zrt_camera* cam, const zrt_params* p) {
  const zrt_vec3* v[4] = {&cam->origin, &cam->lower_left_corner, &cam->horizontal, &cam->vertical};
  float* dst[4] = {a.org, a.llc, a.hor, a.ver};
  for (int k = 0; k < 4; ++k) {
    dst[k][0] = v[k]->x;
    dst[k][1] = v[k]->y;
    dst[k][2] = v[k]->z;
  }
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
// with the grazing-triangle guard, any ray origin and no attenuation rows.
struct TracePlan {
  int kmode = 0;
  bool stk16 = false;
  LdsPlan lp;
};
static TracePlan fill_trace(KArgs& a, const zrt_ctx* c, uint32_t traversal) {
  const int mode = !c->use_bvh ? 0 : traversal == ZRT_TRAVERSAL_REFERENCE ? 2 : traversal == ZRT_TRAVERSAL_BINARY ? 1 : 3;
  const uint32_t stack_depth = mode == 3 ? std::max(c->wide_stack, c->stack_depth) : c->stack_depth;
  const bool qn = mode == 3 && c->q_ok;
  TracePlan t;
  t.kmode = qn ? 8 : mode;
  t.stk16 = mode == 3 ? fast_stk16(c->n_wide, c->n_nodes) : c->n_nodes < 65536;
  t.lp = plan_lds(qn ? c->q_top : c->n_top, c->n_mats, mode, t.stk16, stack_depth, 0, false, false,
                  ZRT_PRNG_XOROSHIRO128, qn ? kQuantNodeF4 : 8u);
  fill_scene(a, c, qn, stack_depth);
  fill_lds(a, t.lp);
  a.check_origins = 1;
  a.guard = c->guard;
  return t;
}
// Its deep stack rows in `ovf`, grown once `st` has drained (an earlier launch may
// still use the old rows), and the bounds the STATS check would read.
static void trace_rows(KArgs& a, const zrt_ctx* c, const TracePlan& t, uint64_t n_lanes, DevBuf<uint8_t>& ovf,
                       hipStream_t st, const char* launch) {
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
  // the probe is the lockstep loop over the full nodes, whatever loop and node
  // format the render launch uses: its own LDS plan (the render's may be the path
  // pool's, whose regions the lockstep loop would read as its lane state and rows)
  const LdsPlan pp = plan_lds(c->n_top, c->n_mats, 3, stk16, a.stack_depth, a.max_depth, false, false, prng);
  // (it reads the material table from LDS only: no schedule for a table past its LDS
  // share - the render then takes the tiles in order)
  if (K.mats_lds_only && !pp.mats_in_lds) return false;
  if (c->probe_partial.n < uint64_t(my_tiles) * 64u) c->probe_partial.alloc(uint64_t(my_tiles) * 64u);
  if (c->probe_scratch.n < uint64_t(kScratchSlots)) c->probe_scratch.alloc(kScratchSlots);
  if (c->tile_cost.n < my_tiles) {
    c->tile_cost.alloc(my_tiles);
    c->cost_sorted.alloc(my_tiles);
    c->tile_order.alloc(my_tiles);
  }
  if (c->tile_ids_n != my_tiles) {
    std::vector<uint32_t> ids(my_tiles);
    for (uint32_t i = 0; i < my_tiles; ++i) ids[i] = i;
    c->tile_ids.upload(ids);
    c->tile_ids_n = my_tiles;
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
  pa.unit_cost = c->tile_cost.p;
  pa.partial = c->probe_partial.p;
  pa.counters = c->probe_scratch.p;
  pa.work_counter = reinterpret_cast<uint32_t*>(c->probe_scratch.p + kWorkSlot);
  const uint32_t pgrid = std::max(1u, std::min(grid, (my_tiles + kBlock / 64 - 1) / (kBlock / 64)));
  pa.n_lanes = pgrid * kBlock;
  fill_tree(pa, c, false);
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
  HIPCHK(hipMemsetAsync(c->probe_scratch.p, 0, kScratchSlots * sizeof(unsigned long long), st));
  void* args[] = {&pa};
  HIPCHK(hipLaunchKernel(probe_kernel(prng, stk16), dim3(pgrid), dim3(kBlock), args, pp.bytes, st));
  size_t bytes = 0;
  HIPCHK(sort_tiles(nullptr, &bytes, c->tile_cost.p, c->cost_sorted.p, c->tile_ids.p, c->tile_order.p, my_tiles, st));
  if (c->sort_temp.n < bytes) c->sort_temp.alloc(bytes);
  HIPCHK(sort_tiles(c->sort_temp.p, &bytes, c->tile_cost.p, c->cost_sorted.p, c->tile_ids.p, c->tile_order.p, my_tiles,
                    st));
  a.tile_order = c->tile_order.p;
  return true;
}

int hip_fail(const HipError& e) {
  return fail(ZRT_E_HIP, e.where + ": " + hipGetErrorString(e.err));
}

constexpr const char* kOverflowMsg = "BVH traversal stack overflow (tree deeper than the stack was sized for)";
constexpr const char* kLayoutMsg = "the kernel refused the wide tree: its layout is not the one the kernel decodes";
constexpr const char* kBoundsMsg = "a global attenuation or stack row index past its buffer (STATS bounds check)";
static const char* device_error_msg(unsigned long long flag) {
  return (flag & kErrLayout) ? kLayoutMsg : (flag & kErrBounds) ? kBoundsMsg : kOverflowMsg;
}

// The device error flag of the context's last launch, copied to pinned host
// memory behind ev_done.  wait: block until the launch is done and report its
// error (every such call does); else (render_tiles' sticky check) report it only
// if the launch has finished and no call has reported it yet.
static int launch_status(zrt_ctx* c, bool wait) {
  if (c->feat_launched && !c->feat_err_reported) {  // a feature launch's error, reported once
    bool done = true;
    if (wait) {
      HIPCHK(hipEventSynchronize(c->feat_done));
    } else if (hipEventQuery(c->feat_done) != hipSuccess) {
      (void)hipGetLastError();  // (not ready is no error of this launch)
      done = false;
    }
    if (done && *c->feat_err_host != 0) {
      c->feat_err_reported = true;
      return fail(ZRT_E_UNSUPPORTED, device_error_msg(*c->feat_err_host));
    }
  }
  if (!c->launched) return ZRT_OK;
  if (wait) {
    HIPCHK(hipEventSynchronize(c->ev_done));
  } else if (hipEventQuery(c->ev_done) != hipSuccess || c->err_reported) {
    return ZRT_OK;
  }
  if (*c->err_host == 0) return ZRT_OK;
  c->err_reported = true;
  return fail(ZRT_E_UNSUPPORTED, device_error_msg(*c->err_host));
}

// A run's earlier passes whose events have completed (wait: all of them) added into
// its render and schedule times; their event sets become spare.  Passes complete in
// the order they were enqueued.
static void fold_pass_times(zrt_ctx* c, bool wait) {
  while (!c->run_pending.empty()) {
    const zrt_ctx::EvSet e = c->run_pending.front();
    if (wait) {
      HIPCHK(hipEventSynchronize(e.e1));
    } else if (hipEventQuery(e.e1) != hipSuccess) {
      (void)hipGetLastError();  // (not ready is no error of this launch)
      break;
    }
    float ms = 0.0f, sched = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, e.pre, e.e1));
    HIPCHK(hipEventElapsedTime(&sched, e.pre, e.e0));
    c->run_render_ms += ms;
    if (e.probed) c->run_sched_ms += sched;
    c->ev_spare.push_back(e);
    c->run_pending.erase(c->run_pending.begin());
  }
}

// A context on `device` holding an uploaded copy of a flattened scene.
std::unique_ptr<zrt_ctx> ctx_on_device(const HostScene& h, int device) {
  std::unique_ptr<zrt_ctx> c(new zrt_ctx);
  c->device = device;
  HIPCHK(hipSetDevice(c->device));
  // a blocking stream: work a caller enqueues on the legacy default stream (NULL,
  // e.g. torch's default stream) after a render on this one waits for it
  HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamDefault));
  HIPCHK(hipEventCreate(&c->ev_pre));
  HIPCHK(hipEventCreate(&c->ev0));
  HIPCHK(hipEventCreate(&c->ev1));
  HIPCHK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->err_host), sizeof(unsigned long long), hipHostMallocDefault));
  *c->err_host = 0;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, c->device));
  c->cu_count = prop.multiProcessorCount;
  upload_scene(c.get(), h);
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
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
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
  } catch (const zrt::HipError& e) {
    return zrt::hip_fail(e);
  } catch (const zrt::Error& e) {
    return fail(e.code, e.what());
  } catch (const std::bad_alloc&) {
    return fail(ZRT_E_NOMEM, "OutOfMemory");
  }
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

// Valid params (zrt::validate_params) are also the context's: its device, its BVH decision.
static int params_fit_ctx(const zrt_ctx* c, const zrt_params* p) {
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  if ((p->bounded_volume_hierarchy != 0 && c->n_prims > 10) != c->use_bvh)
    return fail(ZRT_E_INVALID,
                "params->bounded_volume_hierarchy implies another preprocessSufraces decision (raytrace.zig:124-133) "
                "than the one the context was built with");
  return ZRT_OK;
}

// The launch behind zrt_ctx_render_tiles (run_pass false: the whole frame, resolved by
// finalize_kernel) and zrt_ctx_accum_pass (run_pass true: samples [c->run_done,
// c->run_done + n_samples) of the context's run, p = its params, resolved by
// accumulate_kernel): one launch path and one kernel choice for both.
static int launch_frame(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles, void* hip_stream,
                        bool run_pass, uint32_t n_samples) {
  if (!c || !cam || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  zrt_pass_plan pass{};
  int rc = zrt::plan_pass(p, run_pass ? c->run_done : 0u, run_pass ? n_samples : (p ? p->samples_per_pixel : 0u), &pass);
  if (rc) return rc;
  const bool first = !run_pass || c->run_passes == 0;  // the launch zeroes the counters it adds into
  const bool adapt = run_pass && c->adapt;  // a level of an adaptive run: the active tiles only
  rc = params_fit_ctx(c, p);
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(c->device));
    // a device error of the previous launch that finished meanwhile is reported
    // here (sticky), so a caller that never synchronises through the ABI still sees it
    rc = zrt::launch_status(c, false);
    if (rc) return rc;
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const zrt::Geometry g = zrt::geometry(p);
    const uint32_t my_tiles = zrt::rank_tiles(g, p->rank, p->world_size);
    // the launch decision (zrt::plan_launch; zrt_debug_launch_plan reports the same)
    const zrt::LaunchPlan plan = zrt::plan_launch(c->shape, p);
    const int mode = plan.mode, kmode = plan.kmode;
    const bool diag = (p->flags & ZRT_FLAG_STATS) != 0;
    const bool stk16 = plan.stk16, pool = plan.pool, qn = plan.qn, guard_on = plan.guard_on;
    const uint32_t stack_depth = plan.stack_depth;
    const zrt::LdsPlan& lp = plan.lp;
    // the camera inside the origin bound: so is every ray of the launch (scattered rays start at hits)
    const bool cam_inside = zrt::camera_inside(cam, c->root_c, c->origin_bound);
    void* kfn = zrt::select_kernel(kmode, p->prng, diag, stk16, zrt::lean_launch(plan, diag, cam_inside));
    const size_t lds = lp.bytes;
    int per_cu = 0;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, zrt::kBlock, lds));
    per_cu = std::max(1, std::min(per_cu, 8));
    uint32_t grid = uint32_t(c->cu_count) * uint32_t(per_cu);
    const uint32_t chunk = pass.chunk;
    const uint32_t n_chunks = pass.pass_chunks;
    const uint32_t n_act = adapt ? c->adapt_active : my_tiles;  // tiles the launch hands out
    const uint64_t work64 = uint64_t(n_act) * n_chunks;  // units: (tile, chunk); < 2^32 (plan_pass)
    const uint32_t work = uint32_t(work64);
    // one wave per unit at the start; more waves than units would only idle
    grid = std::max(1u, std::min(grid, (work + (zrt::kBlock / 64) - 1) / (zrt::kBlock / 64)));
    const uint64_t n_partial = uint64_t(my_tiles) * 64u * n_chunks;
    if (c->partial.n < n_partial) c->partial.alloc(n_partial);
    const uint64_t n_lanes = uint64_t(grid) * zrt::kBlock;
    // global attenuation rows: [row][lane], or [path][row] for the path-pool loop
    const uint64_t n_paths = pool ? uint64_t(grid) * zrt::K.block_paths : n_lanes;
    if (n_paths >= (1ull << 32)) return fail(ZRT_E_UNSUPPORTED, "too many paths");
    const zrt::BufNeed need = zrt::buffer_need(lp, p->max_depth, stack_depth, n_paths, n_lanes, stk16);
    if (need.att_elems * sizeof(uint32_t) > (16ull << 30))
      return fail(ZRT_E_UNSUPPORTED, "max_depth too large for the per-lane attenuation stack");
    if (c->att.n < need.att_elems) c->att.alloc(need.att_elems);
    if (first)
      HIPCHK(hipMemsetAsync(c->scratch.p, 0, zrt::kScratchSlots * sizeof(unsigned long long), st));
    else  // a run's later passes add into its counters and keep its error flag: a new work counter only
      HIPCHK(hipMemsetAsync(c->scratch.p + zrt::kWorkSlot, 0, sizeof(unsigned long long), st));
    if (run_pass) {
      // the previous pass's events wait to be added into the run's times (no host wait here)
      if (!first) {
        zrt::fold_pass_times(c, false);  // (frees the sets of passes that have finished)
        if (c->ev_spare.empty()) {
          zrt_ctx::EvSet e;
          HIPCHK(hipEventCreate(&e.pre));
          HIPCHK(hipEventCreate(&e.e0));
          HIPCHK(hipEventCreate(&e.e1));
          c->ev_spare.push_back(e);
        }
        const zrt_ctx::EvSet e = c->ev_spare.back();
        c->ev_spare.pop_back();
        c->run_pending.push_back({c->ev_pre, c->ev0, c->ev1, c->pass_probed});
        c->ev_pre = e.pre;
        c->ev0 = e.e0;
        c->ev1 = e.e1;
      }
      if (first) HIPCHK(hipMemsetAsync(c->accum.p, 0, c->accum.n * sizeof(float4), st));
      if (first && adapt) HIPCHK(hipMemsetAsync(c->tile_done.p, 0, c->tile_done.n * sizeof(uint32_t), st));
    }

    zrt::KArgs a{};
    zrt::fill_scene(a, c, qn, stack_depth);
    zrt::fill_camera(a, cam, p);
    zrt::fill_lds(a, lp);
    a.att = c->att.p;
    a.partial = c->partial.p;
    a.counters = c->scratch.p;
    a.work_counter = reinterpret_cast<uint32_t*>(c->scratch.p + zrt::kWorkSlot);
    a.color_scale = 1.0f / float(pass.samples_after);  // raytrace.zig:157
    a.spp = pass.pass_samples;
    a.max_depth = p->max_depth;
    a.tiles_x = g.tiles_x;
    a.rank = p->rank;
    a.world = p->world_size;
    a.total_work = work;
    a.guard = guard_on ? c->guard : 0.0f;
    a.check_origins = cam_inside ? 0u : 1u;
    if (need.ovf_bytes) {
      if (c->stack_ovf.n < need.ovf_bytes) c->stack_ovf.alloc(need.ovf_bytes);
      a.stack_ovf = c->stack_ovf.p;
    }
    a.n_lanes = uint32_t(n_lanes);
    a.n_paths = uint32_t(n_paths);
    // (a loop that reads the table from LDS only and has none there - the lockstep loop
    // at max_depth 0, which shades nothing - copies none: its plan holds no region for it)
    if (zrt::K.mats_lds_only && kmode == 3 && !lp.mats_in_lds) a.n_mats = 0u;
    a.seed_mix = p->seed * 0x9E3779B97F4A7C15ULL + pass.key_offset;
    if (std::getenv("ZRT_DEBUG_LAUNCH"))
      std::fprintf(stderr, "zrt launch: mode %d stk16 %d grid %u (%d blocks/CU x %d CUs) lds %zu B "
                   "(stack rows %u, top nodes %u @%u, att rows %u @%u, mats %u @%u)\n", mode, int(stk16), grid,
                   per_cu, c->cu_count, lds, lp.stack_rows, a.n_top, lp.top_off, lp.att_rows, lp.att_off,
                   lp.mats_in_lds ? c->n_mats : 0u, lp.mat_off);
    a.chunk = chunk;
    a.n_chunks = n_chunks;
    a.wf_thresh = 48;  // shade once 3/4 of the unit's active lanes are ready (C5: 32 -> 7.32, 48 -> 7.71, 56 -> 7.70 Gray/s)
    if (const char* e = std::getenv("ZRT_WF_THRESH")) a.wf_thresh = std::max(1, std::min(64, std::atoi(e)));
    // the lockstep interval: the BVH loops keep a wave's lanes on one sample (its
    // camera rays coherent); the list loop gains nothing from that (every ray reads
    // the same surfaces) and lets its lanes run through the unit's chunk
    // (C2: 34.1 -> 45.4 Gray/s, profiles/r04/s1)
    a.sync = mode == 0 ? chunk : zrt::K.sync_samples;
    if (const char* e = std::getenv("ZRT_SYNC"))  // A/B: lockstep interval in samples (identical images)
      a.sync = std::max(1u, uint32_t(std::atoi(e)));
    a.n_slots = my_tiles * 64u;

    HIPCHK(hipEventRecord(c->ev_pre, st));
    bool schedule =
        mode == 3 && !(p->flags & ZRT_FLAG_NO_SCHEDULE) && p->samples_per_pixel >= 128 && my_tiles >= 2;
    // (a run decides once, by its cap: its first pass probes, the later ones reuse the
    // order and the probe's counters)
    bool order_hit = false;  // the context holds the order of a probe with this launch's key
    if (schedule && !first) {
      schedule = c->run_ordered;
      if (schedule) a.tile_order = c->tile_order.p;
    } else if (schedule) {
      // (the order cannot change a frame - chunk sums land in fixed slots - so a frame
      // with another seed, sample count or PRNG takes it too; ZRT_ORDER_CACHE=0: A/B)
      zrt_ctx::OrderKey key{};
      key.cam = *cam;
      key.width = p->width;
      key.height = p->height;
      key.max_depth = p->max_depth;
      key.rank = p->rank;
      key.world_size = p->world_size;
      key.traversal = p->traversal;
      key.guard_on = guard_on ? 1u : 0u;
      key.tiles = my_tiles;
      const char* oc = std::getenv("ZRT_ORDER_CACHE");
      order_hit = !(oc && std::atoi(oc) == 0) && c->order_valid &&
                  std::memcmp(&key, &c->order_key, sizeof(key)) == 0;
      if (order_hit) {
        a.tile_order = c->tile_order.p;
      } else {
        c->order_valid = false;  // (the probe overwrites the order, whether or not it completes)
        schedule = zrt::schedule_tiles(c, a, p->prng, stk16, my_tiles, grid, st);
        c->order_key = key;
        c->order_valid = schedule;
      }
    }
    if (run_pass && first) c->run_ordered = schedule;
    if (adapt) {
      // the launch hands out the active list: level 0's is the probe's order where the run
      // is scheduled (else the identity zrt_ctx_adapt_begin uploaded), a later level's is
      // what the previous level's compaction wrote
      uint32_t* list = c->active[c->adapt_cur].p;
      if (first && schedule)
        HIPCHK(hipMemcpyAsync(list, c->tile_order.p, size_t(my_tiles) * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      a.tile_order = list;
    }
    c->pass_probed = schedule && first && !order_hit;
    c->scheduled = schedule;
    // the lockstep loop takes its interval from the probe's lane efficiency (auto_sync;
    // ZRT_SYNC or ZRT_AUTO_SYNC=0: the fixed interval, A/B)
    {
      const char* as = std::getenv("ZRT_AUTO_SYNC");
      const bool auto_on = !std::getenv("ZRT_SYNC") && !(as && std::atoi(as) == 0);
      a.sync_probe = schedule && kmode == 3 && auto_on ? c->probe_scratch.p : nullptr;
    }
    c->scanline_rows = 0;
    if (p->flags & ZRT_FLAG_SCANLINES) {  // (not the probe's: set after it)
      if (c->scanlines.n < size_t(p->height) * 3) c->scanlines.alloc(size_t(p->height) * 3);
      if (first) HIPCHK(hipMemsetAsync(c->scanlines.p, 0, size_t(p->height) * 3 * sizeof(unsigned long long), st));
      a.scanlines = c->scanlines.p;
      c->scanline_rows = p->height;
    }
    if (zrt::K.profile) {
      c->n_waves = grid * (zrt::kBlock / 64);
      if (c->wave_times.n < 2ull * c->n_waves) c->wave_times.alloc(2ull * c->n_waves);
      a.wave_times = c->wave_times.p;
    }
    // every global row the render launch may touch lies inside its buffer (the probe
    // may have grown them): checked on the host, and handed to the STATS flavour's
    // device check
    zrt::check_buffers("render launch", need, c->att.n, c->stack_ovf.n);
    a.att = c->att.p;
    if (need.ovf_bytes) a.stack_ovf = c->stack_ovf.p;
    a.att_cap = c->att.n;
    a.ovf_cap = zrt::ovf_cap_elems(c->stack_ovf.n, stk16);
    if (diag)
      if (const char* e = std::getenv("ZRT_DEBUG_ROW_CAP")) {  // tests: the device check reports a smaller buffer
        const double f = std::atof(e);
        a.att_cap = uint64_t(double(a.att_cap) * f);
        a.ovf_cap = uint64_t(double(a.ovf_cap) * f);
      }
    HIPCHK(hipEventRecord(c->ev0, st));
    if (work > 0) {
      void* args[] = {&a};
      HIPCHK(hipLaunchKernel(kfn, dim3(grid), dim3(zrt::kBlock), args, lds, st));
    }
    HIPCHK(hipEventRecord(c->ev1, st));
    if (run_pass) {
      HIPCHK(hipMemsetAsync(c->metrics.p, 0, zrt::kMetricWords * sizeof(unsigned long long), st));
      // the chunk sums that enter the second moment: all but a ragged last one (zrt.h "the variance plane")
      const uint32_t q_chunks = n_chunks - (pass.last_chunk < chunk ? 1u : 0u);
      if (adapt) {
        // resolve the active tiles, decide (levels 1 .. last - 1), pack the survivors in
        // order into the other list; the host reads their number (zrt_ctx_adapt_level)
        const uint32_t decide = c->adapt_k >= 1 && c->adapt_k + 1 < c->adapt_levels.size() ? 1u : 0u;
        const float prev_scale = c->run_done ? 1.0f / float(c->run_done) : 0.0f;
        HIPCHK(hipMemsetAsync(c->active_count.p, 0, sizeof(uint32_t), st));
        if (n_act > 0) {
          HIPCHK(zrt::launch_resolve(st, c->partial.p, c->accum.p, dev_tiles, c->active[c->adapt_cur].p, n_act, my_tiles,
                                     n_chunks, p->world_size, p->rank, g.tiles_x, g.xbound, p->height, prev_scale,
                                     a.color_scale, q_chunks, c->adapt_a.tolerance, decide, pass.samples_after,
                                     c->tile_done.p,
                                     c->scratch.p + zrt::kErrorSlot, c->metrics.p));
          HIPCHK(zrt::launch_compact(st, c->active[c->adapt_cur].p, n_act, c->tile_done.p,
                                     c->active[c->adapt_cur ^ 1u].p, c->active_count.p));
        }
        HIPCHK(hipMemcpyAsync(c->count_host, c->active_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      } else if (my_tiles > 0) {
        const uint32_t n_slots = my_tiles * 64u;
        const float prev_scale = c->run_done ? 1.0f / float(c->run_done) : 0.0f;
        HIPCHK(zrt::launch_accumulate(st, c->partial.p, c->accum.p, dev_tiles, n_slots, n_chunks, p->world_size, p->rank,
                                      g.tiles_x, g.xbound, p->height, prev_scale, a.color_scale, q_chunks,
                                      c->scratch.p + zrt::kErrorSlot, c->metrics.p));
      }
      HIPCHK(hipMemcpyAsync(c->metrics_host, c->metrics.p, zrt::kMetricWords * sizeof(unsigned long long),
                            hipMemcpyDeviceToHost, st));
    } else if (my_tiles > 0) {
      const uint32_t n_slots = my_tiles * 64u;
      HIPCHK(zrt::launch_finalize(st, c->partial.p, dev_tiles, n_slots, n_chunks, p->world_size, p->rank, g.tiles_x,
                                  g.xbound, p->height, a.color_scale, c->scratch.p + zrt::kErrorSlot));
    }
    HIPCHK(hipMemcpyAsync(c->err_host, c->scratch.p + zrt::kErrorSlot, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ev_done, st));
    c->err_reported = false;
    // count the pixels this rank renders (for samples/pixels counters)
    uint64_t pixels = 0;
    for (uint32_t lt = 0; lt < my_tiles; ++lt) {
      const uint32_t t = lt * p->world_size + p->rank;
      const uint32_t tx = t % g.tiles_x, ty = t / g.tiles_x;
      const uint32_t w = std::min(8u, g.xbound - tx * 8u), h = std::min(8u, p->height - ty * 8u);
      pixels += uint64_t(w) * h;
    }
    c->last_pixels = uint32_t(pixels);
    c->last_spp = pass.samples_after;
    c->last_tiles = my_tiles;
    c->last_rank = p->rank;
    c->last_world = p->world_size;
    c->last_tiles_x = g.tiles_x;
    c->last_xbound = g.xbound;
    c->last_stats = diag;
    c->last_mode = mode;
    c->last_loop = int(zrt::reported_loop(kmode));
    c->last_qn = qn;
    c->last_guard = a.guard;
    c->launched = 1;
    c->run_stats = run_pass;
    c->last_adapt = adapt;
    if (run_pass) {
      c->run_done = pass.samples_after;
      c->run_passes += 1;
      c->pass_samples = pass.pass_samples;
    } else {
      c->run_live = false;  // a plain render overwrites the probe's buffers: it ends the run
    }
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_render_tiles(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_tiles,
                         void* hip_stream) {
  return launch_frame(c, cam, p, dev_tiles, hip_stream, false, 0);
}

int zrt_ctx_accum_begin(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p) {
  if (!c || !cam) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(p);
  if (rc) return rc;
  rc = params_fit_ctx(c, p);
  if (rc) return rc;
  try {
    HIPCHK(hipSetDevice(c->device));
    c->run_live = false;
    const uint64_t n_slots = uint64_t(zrt::rank_tiles(zrt::geometry(p), p->rank, p->world_size)) * 64u;
    if (c->accum.n < n_slots) c->accum.alloc(n_slots);
    if (c->metrics.n < zrt::kMetricWords) c->metrics.alloc(zrt::kMetricWords);
    if (!c->metrics_host) {
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->metrics_host),
                           zrt::kMetricWords * sizeof(unsigned long long), hipHostMallocDefault));
      std::memset(c->metrics_host, 0, zrt::kMetricWords * sizeof(unsigned long long));
    }
    // (a restarted run's unread pass times are dropped; the accumulator, the counters
    // and the error flag are zeroed by the first pass, on its stream)
    for (const zrt_ctx::EvSet& e : c->run_pending) c->ev_spare.push_back(e);
    c->run_pending.clear();
    c->run_render_ms = c->run_sched_ms = 0.0;
    c->run_cam = *cam;
    c->run_p = *p;
    c->run_done = 0;
    c->run_passes = 0;
    c->run_ordered = false;
    c->adapt = false;
    c->run_live = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_accum_pass(zrt_ctx* c, uint32_t n_samples, float* dev_tiles, void* hip_stream) {
  if (!c || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run_live || c->adapt)
    return fail(ZRT_E_INVALID, "no accumulation run is live on this context (zrt_ctx_accum_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  // a device error of an earlier pass is sticky for the run: its accumulator is poisoned
  if (c->run_passes > 0 && hipEventQuery(c->ev_done) == hipSuccess && *c->err_host != 0) {
    c->err_reported = true;
    return fail(ZRT_E_UNSUPPORTED, zrt::device_error_msg(*c->err_host));
  }
  (void)hipGetLastError();
  return launch_frame(c, &c->run_cam, &c->run_p, dev_tiles, hip_stream, true, n_samples);
}

int zrt_ctx_accum_info(zrt_ctx* c, zrt_pass_info* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->launched || !c->run_stats) return fail(ZRT_E_INVALID, "the context's last launch was not a zrt_ctx_accum_pass");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_done));
    std::memset(out, 0, sizeof(*out));
    out->samples_done = c->run_done;
    out->pass_samples = c->pass_samples;
    uint32_t bits = 0;  // the shards' sum and maximum
    for (uint32_t k = 0; k < zrt::kMetricShards; ++k) {
      out->changed_pixels += c->metrics_host[k * zrt::kMetricStride];
      bits = std::max(bits, uint32_t(c->metrics_host[k * zrt::kMetricStride + 1]));
    }
    std::memcpy(&out->max_abs_change, &bits, 4);
    float ms = 0.0f, sched = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_pre, c->ev1));
    HIPCHK(hipEventElapsedTime(&sched, c->ev_pre, c->ev0));
    out->render_ms = ms;
    out->schedule_ms = c->pass_probed ? sched : 0.0f;
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
    c->run_live = false;
    const uint32_t my_tiles = zrt::rank_tiles(zrt::geometry(p), p->rank, p->world_size);
    // (no level of an earlier run is in flight: zrt_ctx_adapt_level waits for its own)
    std::vector<uint32_t> ids(my_tiles);
    for (uint32_t i = 0; i < my_tiles; ++i) ids[i] = i;
    if (c->active[0].n < my_tiles || c->active[1].n < my_tiles || c->tile_done.n < my_tiles) {
      c->active[0].alloc(my_tiles);
      c->active[1].alloc(my_tiles);
      c->tile_done.alloc(my_tiles);
    }
    if (my_tiles)
      HIPCHK(hipMemcpy(c->active[0].p, ids.data(), size_t(my_tiles) * sizeof(uint32_t), hipMemcpyHostToDevice));
    if (c->active_count.n < 1) c->active_count.alloc(1);
    if (!c->count_host)
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->count_host), sizeof(uint32_t), hipHostMallocDefault));
    *c->count_host = 0;
    c->adapt_a = *ad;
    c->adapt_levels = levels;
    c->adapt_k = 0;
    c->adapt_cur = 0;
    c->adapt_active = my_tiles;
    c->adapt_samples = 0;
    c->adapt_tiles = nullptr;
    c->adapt = true;
    c->run_live = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_adapt_level(zrt_ctx* c, float* dev_tiles, void* hip_stream, zrt_level_info* out) {
  if (!c || !dev_tiles) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run_live || !c->adapt)
    return fail(ZRT_E_INVALID, "no adaptive run is live on this context (zrt_ctx_adapt_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  // a device error of an earlier level is sticky for the run (every level is waited for)
  if (c->run_passes > 0 && *c->err_host != 0) {
    c->err_reported = true;
    return fail(ZRT_E_UNSUPPORTED, zrt::device_error_msg(*c->err_host));
  }
  if (c->adapt_k >= c->adapt_levels.size()) return fail(ZRT_E_INVALID, "the adaptive run has rendered its last level");
  if (c->adapt_active == 0 && c->run_passes > 0) return fail(ZRT_E_INVALID, "no tile of the adaptive run is active");
  if (c->adapt_tiles && c->adapt_tiles != dev_tiles)
    return fail(ZRT_E_INVALID, "dev_tiles differs from the run's earlier levels' (frozen tiles live there)");
  const uint32_t level = c->adapt_levels[c->adapt_k], rendered = c->adapt_active;
  const uint32_t level_samples = level - c->run_done;
  const int rc = launch_frame(c, &c->run_cam, &c->run_p, dev_tiles, hip_stream, true, level_samples);
  if (rc) return rc;
  try {
    HIPCHK(hipEventSynchronize(c->ev_done));  // the one wait of the level: the surviving count is here
    c->adapt_tiles = dev_tiles;
    c->adapt_k += 1;
    c->adapt_cur ^= 1u;
    c->adapt_active = c->adapt_k < c->adapt_levels.size() ? *c->count_host : 0u;
    uint64_t pixels = 0, changed = 0;
    uint32_t bits = 0;
    for (uint32_t k = 0; k < zrt::kMetricShards; ++k) {
      changed += c->metrics_host[k * zrt::kMetricStride];
      bits = std::max(bits, uint32_t(c->metrics_host[k * zrt::kMetricStride + 1]));
      pixels += c->metrics_host[k * zrt::kMetricStride + 2];
    }
    if (*c->err_host == 0) c->adapt_samples += pixels * level_samples;
    if (out) {
      std::memset(out, 0, sizeof(*out));
      out->level_samples = level;
      out->tiles_rendered = rendered;
      out->tiles_active_after = c->adapt_active;
      out->samples_rendered = pixels * level_samples;
      out->changed_pixels = changed;
      std::memcpy(&out->max_abs_change, &bits, 4);
      float ms = 0.0f, sched = 0.0f;
      HIPCHK(hipEventElapsedTime(&ms, c->ev_pre, c->ev1));
      HIPCHK(hipEventElapsedTime(&sched, c->ev_pre, c->ev0));
      out->render_ms = ms;
      out->schedule_ms = c->pass_probed ? sched : 0.0f;
    }
    return zrt::launch_status(c, true);
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_adapt_samples(zrt_ctx* c, uint32_t* per_tile, uint32_t cap_tiles) {
  if (!c || !per_tile) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run_live || !c->adapt) return fail(ZRT_E_INVALID, "no adaptive run is live on this context");
  const uint32_t my_tiles = zrt::rank_tiles(zrt::geometry(&c->run_p), c->run_p.rank, c->run_p.world_size);
  if (cap_tiles < my_tiles) return fail(ZRT_E_INVALID, "per_tile holds fewer entries than the rank has tiles");
  try {
    HIPCHK(hipSetDevice(c->device));
    if (c->run_passes == 0) {
      std::fill(per_tile, per_tile + my_tiles, 0u);
      return ZRT_OK;
    }
    HIPCHK(hipEventSynchronize(c->ev_done));
    if (my_tiles)
      HIPCHK(hipMemcpy(per_tile, c->tile_done.p, size_t(my_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < my_tiles; ++i) per_tile[i] &= ~zrt::kTileFrozen;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_stats(zrt_ctx* c, zrt_stats* out) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->launched) return fail(ZRT_E_INVALID, "zrt_ctx_stats before any zrt_ctx_render_tiles");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_done));
    unsigned long long h[zrt::kScratchSlots] = {0};
    HIPCHK(hipMemcpy(h, c->scratch.p, sizeof(h), hipMemcpyDeviceToHost));
    if (c->scanline_rows) {  // ZRT_FLAG_SCANLINES: the launch counted these three per row only
      std::vector<unsigned long long> rows(size_t(c->scanline_rows) * 3);
      HIPCHK(hipMemcpy(rows.data(), c->scanlines.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
      for (size_t y = 0; y < c->scanline_rows; ++y) {
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
    const uint64_t samples = c->last_adapt ? c->adapt_samples : uint64_t(c->last_pixels) * c->last_spp;
    out->rays_processed = c->last_stats ? h[zrt::kRays] : samples + h[zrt::kReflections] - h[zrt::kDepthHits];
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
    out->node_bytes = c->last_mode == 3 ? (c->last_qn ? 64 : 128) : 32;
    out->wide_nodes = c->n_wide;
    out->sampling_loop = uint32_t(c->last_loop);
    out->guard = c->last_guard;
    out->texel_bytes = c->texel_bytes;
    out->pixels_processed = c->last_pixels;
    out->samples_processed = samples;
    out->preprocess_ms = c->preprocess_ms;
    out->upload_ms = c->upload_ms;
    float ms = 0.0f, sched = 0.0f;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_pre, c->ev1));
    HIPCHK(hipEventElapsedTime(&sched, c->ev_pre, c->ev0));
    out->render_ms = ms;
    out->schedule_ms = c->pass_probed ? sched : 0.0f;  // (0 when a kept order was reused)
    if (c->run_stats) {  // a run: the sums over its passes (the counters above were never re-zeroed)
      zrt::fold_pass_times(c, true);
      out->render_ms = c->run_render_ms + ms;
      out->schedule_ms = float(c->run_sched_ms + (c->pass_probed ? sched : 0.0f));
    }
    out->used_bvh = c->use_bvh ? 1 : 0;
    out->bvh_nodes = c->n_nodes;
    out->bvh_max_depth = c->bvh_depth;
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

namespace zrt {
// The per-row Progress counters of c's last launch (ZRT_FLAG_SCANLINES) added
// into out[0 .. height): this rank's pixels, samples and rays of each row and
// the three counters the kernel counted per row.
int add_scanlines(zrt_ctx* c, zrt_scanline* out, uint32_t height) {
  if (!c->launched || c->scanline_rows == 0)
    return fail(ZRT_E_INVALID, "the last launch did not count scanlines (ZRT_FLAG_SCANLINES)");
  if (height != c->scanline_rows) return fail(ZRT_E_INVALID, "height differs from the last launch's");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->ev_done));
  std::vector<unsigned long long> rows(size_t(height) * 3);
  HIPCHK(hipMemcpy(rows.data(), c->scanlines.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  std::vector<uint32_t> done;  // an adaptive run: samples per pixel of each tile
  if (c->last_adapt) {
    done.resize(std::max(1u, c->last_tiles));
    HIPCHK(hipMemcpy(done.data(), c->tile_done.p, size_t(c->last_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  std::vector<uint64_t> row_samples(height, 0);
  for (uint32_t lt = 0; lt < c->last_tiles; ++lt) {  // pixels of this rank's tiles, per row
    const uint32_t t = lt * c->last_world + c->last_rank;
    const uint32_t tx = t % c->last_tiles_x, ty = t / c->last_tiles_x;
    const uint32_t w = std::min(8u, c->last_xbound - tx * 8u);
    const uint32_t spp = c->last_adapt ? done[lt] & ~kTileFrozen : c->last_spp;
    for (uint32_t y = ty * 8u; y < std::min(height, ty * 8u + 8u); ++y) {
      out[y].pixels += w;
      row_samples[y] += uint64_t(w) * spp;
    }
  }
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

int zrt_ctx_debug_counters(zrt_ctx* c, uint64_t* out, uint32_t n) {
  if (!c || !out) return fail(ZRT_E_INVALID, "null argument");
  if (!c->launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_done));
    unsigned long long h[zrt::kScratchSlots] = {0};
    HIPCHK(hipMemcpy(h, c->scratch.p, sizeof(h), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n && i < uint32_t(zrt::kScratchSlots); ++i) out[i] = h[i];
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_debug_wave_times(zrt_ctx* c, uint64_t* out, uint32_t cap, uint32_t* n_waves) {
  if (!c || !n_waves) return fail(ZRT_E_INVALID, "null argument");
  try {
    HIPCHK(hipSetDevice(c->device));
    if (c->launched) HIPCHK(hipEventSynchronize(c->ev_done));
    *n_waves = zrt::K.profile ? c->n_waves : 0u;
    const size_t n = std::min<size_t>(cap / 2, *n_waves);
    if (n && out) HIPCHK(hipMemcpy(out, c->wave_times.p, 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_debug_schedule(zrt_ctx* c, uint32_t* costs, uint32_t* order, uint32_t cap, uint32_t* n_tiles) {
  if (!c || !n_tiles) return fail(ZRT_E_INVALID, "null argument");
  if (!c->launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev_done));
    *n_tiles = c->scheduled ? c->tile_ids_n : 0u;
    const size_t n = std::min<size_t>(cap, *n_tiles);
    if (n && costs) HIPCHK(hipMemcpy(costs, c->tile_cost.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n && order) HIPCHK(hipMemcpy(order, c->tile_order.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_last_kernel_ms(zrt_ctx* c, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!c->launched) return fail(ZRT_E_INVALID, "no kernel launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ev1));
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, c->ev0, c->ev1));
    *ms = f;
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

// ---- the variance plane of the live run (zrt.h "the variance plane") ----------
int zrt_ctx_accum_variance(zrt_ctx* c, float* dev_tiles_var, void* hip_stream) {
  if (!c || !dev_tiles_var) return fail(ZRT_E_INVALID, "null argument");
  if (!c->run_live)
    return fail(ZRT_E_INVALID, "no run is live on this context (zrt_ctx_accum_begin / zrt_ctx_adapt_begin; a "
                               "zrt_ctx_render_tiles ends the run)");
  if (c->run_passes == 0) return fail(ZRT_E_INVALID, "variance: the run has rendered no pass yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const zrt_params* p = &c->run_p;
    const zrt::Geometry g = zrt::geometry(p);
    const uint32_t my_tiles = zrt::rank_tiles(g, p->rank, p->world_size);
    const uint32_t n_slots = my_tiles * 64u;
    HIPCHK(hipEventSynchronize(c->ev_done));  // the last pass: its error flag, an adaptive run's tile counts
    const bool dev_err = *c->err_host != 0;
    c->var_plan_host.assign(std::max(1u, my_tiles), make_float2(0.0f, 0.0f));
    if (!dev_err) {
      zrt_variance_plan vp{};
      if (c->adapt) {
        std::vector<uint32_t> done(std::max(1u, my_tiles));
        if (my_tiles)
          HIPCHK(hipMemcpy(done.data(), c->tile_done.p, size_t(my_tiles) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint32_t last_n = 0;
        for (uint32_t lt = 0; lt < my_tiles; ++lt) {
          const uint32_t n = done[lt] & ~zrt::kTileFrozen;
          if (n != last_n) {  // (ik and sc per distinct k)
            const int rc = zrt::plan_variance(p, n, &vp);
            if (rc) return rc;
            last_n = n;
          }
          c->var_plan_host[lt] = make_float2(vp.ik, vp.sc);
        }
      } else {
        const int rc = zrt::plan_variance(p, c->run_done, &vp);
        if (rc) return rc;
        for (uint32_t lt = 0; lt < my_tiles; ++lt) c->var_plan_host[lt] = make_float2(vp.ik, vp.sc);
      }
    }
    if (c->var_plan.n < c->var_plan_host.size()) c->var_plan.alloc(c->var_plan_host.size());
    // (a blocking copy: the table may be rewritten by the next call)
    HIPCHK(hipMemcpy(c->var_plan.p, c->var_plan_host.data(), c->var_plan_host.size() * sizeof(float2),
                     hipMemcpyHostToDevice));
    if (n_slots)
      HIPCHK(zrt::launch_variance(st, c->accum.p, c->var_plan.p, dev_tiles_var, n_slots, p->world_size, p->rank,
                                  g.tiles_x, g.xbound, p->height, c->scratch.p + zrt::kErrorSlot));
    if (dev_err) {
      c->err_reported = true;
      return fail(ZRT_E_UNSUPPORTED, zrt::device_error_msg(*c->err_host));
    }
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// ---- first-hit feature buffers (zrt.h "denoising") ---------------------------
int zrt_ctx_features(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, float* dev_features, void* hip_stream) {
  if (!c || !cam || !dev_features) return fail(ZRT_E_INVALID, "null argument");
  int rc = zrt::validate_params(p);
  if (rc) return rc;
  rc = params_fit_ctx(c, p);
  if (rc) return rc;
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "dev_features must be 16-byte aligned");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const uint32_t tiles = ((p->width + 7u) / 8u) * ((p->height + 7u) / 8u);
    const uint32_t grid = (tiles + zrt::kBlock / 64 - 1) / (zrt::kBlock / 64);
    const uint64_t n_lanes = uint64_t(grid) * zrt::kBlock;
    if (c->feat_slot_prim.n < c->slot_to_prim.size() || c->feat_slot_prim.p == nullptr)
      c->feat_slot_prim.upload(c->slot_to_prim);
    if (!c->feat_done) {
      HIPCHK(hipEventCreateWithFlags(&c->feat_done, hipEventDisableTiming));
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->feat_err_host), sizeof(unsigned long long),
                           hipHostMallocDefault));
      *c->feat_err_host = 0;
    }
    // the context's error flag: what a render launch left there stays (a run's flag is
    // sticky); before the first launch the slots hold nothing yet
    if (!c->launched && !c->feat_launched)
      HIPCHK(hipMemsetAsync(c->scratch.p, 0, zrt::kScratchSlots * sizeof(unsigned long long), st));
    zrt::KArgs a{};
    const zrt::TracePlan t = zrt::fill_trace(a, c, p->traversal);
    zrt::fill_camera(a, cam, p);
    zrt::trace_rows(a, c, t, n_lanes, c->feat_ovf, st, "feature launch");
    void* fn = zrt::features_kernel_ptr(t.kmode, t.stk16);
    const uint32_t* sp = c->feat_slot_prim.p;
    float4* out = reinterpret_cast<float4*>(dev_features);
    void* args[] = {&a, &sp, &out};
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(zrt::kBlock), args, t.lp.bytes, st));
    const uint64_t n_f4 = 2ull * p->width * p->height;
    HIPCHK(zrt::launch_features_error(st, out, n_f4, c->scratch.p + zrt::kErrorSlot));
    HIPCHK(hipMemcpyAsync(c->feat_err_host, c->scratch.p + zrt::kErrorSlot, sizeof(unsigned long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->feat_done, st));
    c->feat_launched = true;
    c->feat_err_reported = false;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

// ---- denoising (zrt.h "denoising"; the kernels: denoise.hip) ----------------
// the default sigmas: the winner of tools/denoise_probe.py's grid of powers of two
// (profiles/r10/denoise/defaults.json)
#define ZRT_DN_SIGMA_COLOR 2.0f
#define ZRT_DN_SIGMA_NORMAL 0.125f
#define ZRT_DN_SIGMA_ALBEDO 0x1p-12f
#define ZRT_DN_SIGMA_DEPTH 0.015625f
int zrt_denoise_defaults(zrt_denoise* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  *out = zrt_denoise{};
  out->iterations = ZRT_DEFAULT_DENOISE_ITERATIONS;
  // the winner of tools/denoise_probe.py's grid (profiles/r10/denoise/defaults.json)
  out->sigma_color = ZRT_DN_SIGMA_COLOR;
  out->sigma_normal = ZRT_DN_SIGMA_NORMAL;
  out->sigma_albedo = ZRT_DN_SIGMA_ALBEDO;
  out->sigma_depth = ZRT_DN_SIGMA_DEPTH;
  return ZRT_OK;
}

int zrt_ctx_denoise(zrt_ctx* c, const zrt_params* p, const zrt_denoise* dn, const float* dev_frame,
                    const float* dev_features, float* dev_out, void* hip_stream) {
  zrt::DenoiseLaunch l{};
  int rc = zrt::plan_denoise(p, dn, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  if (dev_out && static_cast<const float*>(dev_out) == dev_frame)
    return fail(ZRT_E_INVALID, "denoise: dev_out must not be dev_frame");
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "denoise: dev_features must be 16-byte aligned");
  if (!c || !dev_frame || !dev_features || !dev_out) return fail(ZRT_E_INVALID, "null argument");
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t plane = size_t(l.n) * l.n;
    for (zrt::DevBuf<float4>& b : c->dn_buf)
      if (b.n < plane) b.alloc(plane);
    if (!c->dn_ev0) {
      HIPCHK(hipEventCreate(&c->dn_ev0));
      HIPCHK(hipEventCreate(&c->dn_ev1));
    }
    HIPCHK(hipEventRecord(c->dn_ev0, st));
    HIPCHK(zrt::denoise_enqueue(l, dev_frame, reinterpret_cast<const float4*>(dev_features), dev_out, c->dn_buf[0].p,
                                c->dn_buf[1].p, st));
    HIPCHK(hipEventRecord(c->dn_ev1, st));
    c->dn_launched = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
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
  *out = zrt_denoise{};
  out->iterations = ZRT_DEFAULT_DENOISE_ITERATIONS;
  out->sigma_color = ZRT_DG_SIGMA_COLOR;
  out->sigma_normal = ZRT_DG_SIGMA_NORMAL;
  out->sigma_albedo = ZRT_DG_SIGMA_ALBEDO;
  out->sigma_depth = ZRT_DG_SIGMA_DEPTH;
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
  if (dev_out && static_cast<const float*>(dev_out) == dev_frame)
    return fail(ZRT_E_INVALID, "denoise: dev_out must not be dev_frame");
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "denoise: dev_features must be 16-byte aligned");
  if (!dev_variance) return fail(ZRT_E_INVALID, "denoise: dev_variance is null");
  if (dev_out_variance && static_cast<const float*>(dev_out_variance) == dev_variance)
    return fail(ZRT_E_INVALID, "denoise: dev_out_variance must not be dev_variance");
  if (!c || !dev_frame || !dev_features || !dev_out) return fail(ZRT_E_INVALID, "null argument");
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t plane = size_t(l.n) * l.n;
    for (zrt::DevBuf<float4>& b : c->dn_buf)
      if (b.n < plane) b.alloc(plane);
    if (!c->dn_ev0) {
      HIPCHK(hipEventCreate(&c->dn_ev0));
      HIPCHK(hipEventCreate(&c->dn_ev1));
    }
    HIPCHK(hipEventRecord(c->dn_ev0, st));
    HIPCHK(zrt::denoise_guided_enqueue(l, dn->sigma_color, (flags & ZRT_DN_DEMODULATE) != 0, dev_frame,
                                       reinterpret_cast<const float4*>(dev_features), dev_variance, dev_out,
                                       dev_out_variance, c->dn_buf[0].p, c->dn_buf[1].p, st));
    HIPCHK(hipEventRecord(c->dn_ev1, st));
    c->dn_launched = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_denoise_ms(zrt_ctx* c, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!c->dn_launched) return fail(ZRT_E_INVALID, "no denoise launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->dn_ev1));
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, c->dn_ev0, c->dn_ev1));
    *ms = f;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
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
  *out = zrt_temporal{};
  out->alpha_min = ZRT_TA_ALPHA_MIN;
  out->max_history = ZRT_TA_MAX_HISTORY;
  out->sigma_normal = ZRT_TA_SIGMA_NORMAL;
  out->sigma_depth = ZRT_TA_SIGMA_DEPTH;
  out->flags = ZRT_TA_FLAGS;
  return ZRT_OK;
}

int zrt_ctx_temporal(zrt_ctx* c, const zrt_camera* cam, const zrt_params* p, const zrt_temporal* tp,
                     const float* dev_frame, const float* dev_features, const float* dev_variance, float* dev_out,
                     float* dev_out_variance, uint32_t* dev_out_len, void* hip_stream) {
  zrt::TemporalLaunch l{};
  int rc = zrt::plan_temporal(p, tp, &l);  // (the refusals that need no context come first)
  if (rc) return rc;
  if (dev_out && static_cast<const float*>(dev_out) == dev_frame)
    return fail(ZRT_E_INVALID, "temporal: dev_out must not be dev_frame");
  if (reinterpret_cast<uintptr_t>(dev_features) & 15u)
    return fail(ZRT_E_INVALID, "temporal: dev_features must be 16-byte aligned");
  if (!dev_variance) return fail(ZRT_E_INVALID, "temporal: dev_variance is null");
  if (dev_out_variance && static_cast<const float*>(dev_out_variance) == dev_variance)
    return fail(ZRT_E_INVALID, "temporal: dev_out_variance must not be dev_variance");
  if (!c || !cam || !dev_frame || !dev_features || !dev_out) return fail(ZRT_E_INVALID, "null argument");
  if (int(p->device) != c->device)
    return fail(ZRT_E_INVALID, "params->device differs from the device the context was created on");
  try {
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    const size_t plane = size_t(l.n) * l.n;
    if (c->ta_width != p->width || c->ta_height != p->height || c->ta_hist[0].n < plane) {
      for (int k = 0; k < 2; ++k) {  // (hipFree waits for the frames in flight)
        c->ta_hist[k].alloc(plane);
        c->ta_feat[k].alloc(2 * plane);
        c->ta_len[k].alloc(plane);
      }
      c->ta_width = p->width;
      c->ta_height = p->height;
      c->ta_live = false;
    }
    if (c->ta_demod != l.demod) c->ta_live = false;
    if (c->ta_live) {
      zrt_reproject_plan rp{};
      rc = zrt::plan_reproject(&c->ta_cam, p, &rp);
      if (rc) return rc;
      l.history = rp.valid;
      l.static_cam = std::memcmp(cam, &c->ta_cam, sizeof(zrt_camera)) == 0 ? 1u : 0u;
      const zrt_vec3* src[4] = {&rp.origin, &rp.rn, &rp.ru, &rp.rv};
      float* dst[4] = {l.porg, l.rn, l.ru, l.rv};
      for (int k = 0; k < 4; ++k) {
        dst[k][0] = src[k]->x;
        dst[k][1] = src[k]->y;
        dst[k][2] = src[k]->z;
      }
    }
    {
      const zrt_vec3* src[4] = {&cam->origin, &cam->lower_left_corner, &cam->horizontal, &cam->vertical};
      float* dst[4] = {l.org, l.llc, l.hor, l.ver};
      for (int k = 0; k < 4; ++k) {
        dst[k][0] = src[k]->x;
        dst[k][1] = src[k]->y;
        dst[k][2] = src[k]->z;
      }
    }
    if (!c->ta_ev0) {
      HIPCHK(hipEventCreate(&c->ta_ev0));
      HIPCHK(hipEventCreate(&c->ta_ev1));
    }
    const uint32_t cur = c->ta_cur, nxt = cur ^ 1u;
    const zrt::TemporalPlanes prev{c->ta_hist[cur].p, c->ta_feat[cur].p, c->ta_len[cur].p};
    const zrt::TemporalPlanes next{c->ta_hist[nxt].p, c->ta_feat[nxt].p, c->ta_len[nxt].p};
    HIPCHK(hipEventRecord(c->ta_ev0, st));
    HIPCHK(zrt::temporal_enqueue(l, dev_frame, reinterpret_cast<const float4*>(dev_features), dev_variance, prev, next,
                                 dev_out, dev_out_variance, dev_out_len, st));
    HIPCHK(hipEventRecord(c->ta_ev1, st));
    c->ta_cur = nxt;
    c->ta_cam = *cam;
    c->ta_demod = l.demod;
    c->ta_live = true;
    c->ta_launched = true;
    return ZRT_OK;
  }
  ZRT_CATCH_ALL
}

int zrt_ctx_temporal_reset(zrt_ctx* c) {
  if (!c) return fail(ZRT_E_INVALID, "null argument");
  c->ta_live = false;
  return ZRT_OK;
}

int zrt_ctx_temporal_ms(zrt_ctx* c, double* ms) {
  if (!c || !ms) return fail(ZRT_E_INVALID, "null argument");
  if (!c->ta_launched) return fail(ZRT_E_INVALID, "no temporal step launched on this context yet");
  try {
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->ta_ev1));
    float f = 0.0f;
    HIPCHK(hipEventElapsedTime(&f, c->ta_ev0, c->ta_ev1));
    *ms = f;
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
      out_prim[i] = slot[i] < 0 ? -1 : int32_t(c->slot_to_prim[size_t(slot[i])]);
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
