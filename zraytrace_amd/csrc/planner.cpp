// planner.cpp - what a launch needs decided before any device is touched:
// validation, tile geometry, the environment knobs, the block's LDS plan, the
// global rows a launch needs, the launch / pass / adaptive / denoise plans.
// No HIP call; the kernels' build values come from kernel_config().
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>

#include "accel_build.hpp"
#include "bvh_build.hpp"
#include "host.hpp"

namespace zrt {
static const KernelConfig& K = kernel_config();

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int validate_scene(const zrt_scene* s) {
  if (!s) return fail(ZRT_E_INVALID, "scene is null");
  if (s->n_prims && !s->prims) return fail(ZRT_E_INVALID, "prims is null");
  if (s->n_materials && !s->materials) return fail(ZRT_E_INVALID, "materials is null");
  if (s->n_textures && !s->textures) return fail(ZRT_E_INVALID, "textures is null");
  if (s->n_images && !s->images) return fail(ZRT_E_INVALID, "images is null");
  if (s->n_prims >= (1u << 29)) return fail(ZRT_E_UNSUPPORTED, "more than 2^29 primitives");
  for (uint32_t i = 0; i < s->n_prims; ++i) {
    const zrt_prim& p = s->prims[i];
    if (p.kind != ZRT_PRIM_SPHERE && p.kind != ZRT_PRIM_TRIANGLE) return fail(ZRT_E_INVALID, "unknown primitive kind");
    if (p.material >= s->n_materials) return fail(ZRT_E_INVALID, "material index out of range");
    // A NaN midpoint (a NaN bound, or a box from -inf to +inf: a NaN centre or radius, an
    // infinite radius) has no place under the `<` the reference sorts midpoints by
    // (bvh.zig:85-120): the tree then depends on the sort's algorithm, not on the scene.
    const Box b = prim_box(p);
    if (std::isnan(b.mid[0]) || std::isnan(b.mid[1]) || std::isnan(b.mid[2]))
      return fail(ZRT_E_UNSUPPORTED, "primitive " + std::to_string(i) +
                                         ": its bounding box has a NaN midpoint (a NaN or unbounded coordinate), "
                                         "which the reference's BVH sort does not order");
  }
  for (uint32_t i = 0; i < s->n_materials; ++i) {
    const zrt_material& m = s->materials[i];
    if (m.kind > ZRT_MAT_DIELECTRIC) return fail(ZRT_E_INVALID, "unknown material kind");
    if (m.kind != ZRT_MAT_DIELECTRIC) {
      if (m.texture >= s->n_textures) return fail(ZRT_E_INVALID, "texture index out of range");
      const zrt_texture& t = s->textures[m.texture];
      if (t.kind > ZRT_TEX_IMAGE) return fail(ZRT_E_INVALID, "unknown texture kind");
      if (t.kind == ZRT_TEX_IMAGE) {
        if (t.image >= s->n_images) return fail(ZRT_E_INVALID, "image index out of range");
        const zrt_image& im = s->images[t.image];
        if (!im.pixels || im.width == 0 || im.height == 0) return fail(ZRT_E_INVALID, "empty image");
      }
    }
  }
  return ZRT_OK;
}

int validate_params(const zrt_params* p) {
  if (!p) return fail(ZRT_E_INVALID, "params is null");
  if (p->width == 0 || p->height == 0 || p->samples_per_pixel == 0)
    return fail(ZRT_E_INVALID, "width, height and samples_per_pixel must be > 0");
  if (p->width > 65535 || p->height > 65535 || p->samples_per_pixel > 65535 || p->max_depth > 65535)
    return fail(ZRT_E_INVALID, "RenderParams fields are u16 (raytrace.zig:102-108)");
  if (p->height > p->width)
    return fail(ZRT_E_INVALID,
                "height > width: raytrace.zig:168 iterates x over image.height and would write past the image");
  if (p->rng_mode != ZRT_RNG_COUNTER)
    return fail(ZRT_E_UNSUPPORTED,
                "the single sequential reference stream cannot be split across GPU lanes; use ZRT_RNG_COUNTER");
  if (p->prng > ZRT_PRNG_XOSHIRO256) return fail(ZRT_E_INVALID, "unknown prng");
  if (p->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  if (p->world_size == 0 || p->rank >= p->world_size) return fail(ZRT_E_INVALID, "rank must be < world_size");
  if (p->sample_chunk > 65535) return fail(ZRT_E_INVALID, "sample_chunk must be <= 65535");
  return ZRT_OK;
}

Geometry geometry(const zrt_params* p) {
  Geometry g;
  g.xbound = p->height;  // raytrace.zig:168: `while (x < image.height)`
  g.tiles_x = (g.xbound + 7) / 8;
  g.tiles_y = (p->height + 7) / 8;
  g.n_tiles = g.tiles_x * g.tiles_y;
  return g;
}
uint32_t rank_tiles(const Geometry& g, uint32_t rank, uint32_t world) {
  return g.n_tiles > rank ? (g.n_tiles - rank + world - 1) / world : 0;
}
void for_rank_tiles(const Geometry& g, uint32_t height, uint32_t rank, uint32_t world,
                    const std::function<void(uint32_t lt, uint32_t w, uint32_t h, uint32_t y0)>& f) {
  const uint32_t n = rank_tiles(g, rank, world);
  for (uint32_t lt = 0; lt < n; ++lt) {
    const uint32_t t = lt * world + rank, tx = t % g.tiles_x, ty = t / g.tiles_x;
    f(lt, std::min(8u, g.xbound - tx * 8u), std::min(8u, height - ty * 8u), ty * 8u);
  }
}

// The wavefront loop (render_loop_wf) for this scene?  ZRT_WF=0/1 forces it.
// It doubles the traversal lane efficiency where traversal lengths diverge
// (C3 0.29 -> 0.59, C5 0.22 -> 0.41), but the FAST loop is bound by its
// per-lane node fetches (vector memory), not by VALU lane slots, so that buys
// little time: C5 +2.6 %, C3 -3 .. +1 %, and on the bunny, whose lockstep
// camera rays share cache lines, it costs a third.  Default:
// trees too large for the 16-bit stack (million-triangle meshes, C5).
static bool use_wavefront(bool stk16) {
  if (const char* e = std::getenv("ZRT_WF")) return std::atoi(e) != 0;
  return !stk16;
}
// Per-axis margins (wide_iter) in waves with a lane whose max_k |1/d_k| exceeds
// this; ZRT_PAXIS_M overrides (the tests set 0: every wave takes them)
float paxis_threshold() {
  if (const char* e = std::getenv("ZRT_PAXIS_M")) return float(std::atof(e));
  return kernel_config().paxis_m;
}
// A ray's octant copy starts oct * stride_f4 float4s into the nodes and oct * n_top *
// node_f4 into the LDS top levels (render.hip wide_view).  The kernels form both by
// a 24-bit multiply (oct_times), which reads the low 24 bits of each
// factor only: a tree whose stride or top levels reach 2^24 float4s (2 M full nodes
// per copy; the C5 mesh has 3.7 M float4s) is refused before anything is uploaded.
void check_octant_offsets(uint32_t stride_f4, uint32_t n_top, uint32_t node_f4) {
  constexpr uint64_t lim = 1ull << 24;
  const uint64_t top = uint64_t(n_top) * node_f4;
  if (stride_f4 >= lim || top >= lim)
    throw Error(ZRT_E_UNSUPPORTED, "wide tree too large for the kernels' 24-bit octant offsets: " +
                                       std::to_string(stride_f4) + " float4s per octant copy, " + std::to_string(top) +
                                       " in its top levels (each must be below 2^24)");
}
// The path-pool loop (render_loop_pool, MODE 5) instead of the wavefront loop?
// ZRT_POOL=0/1 forces it.  Default: the wavefront loop's cases (trees past the
// 16-bit stack), where it is 4 % faster at C5's full size (8.30 -> 8.65 Gray/s,
// profiles/r03/ab5); on the teapot (C3) and the bunny (C4) the lockstep loop
// stays ahead (14.7 vs 14.3, 50.5 vs 29.4 Gray/s).
static bool use_pool(bool stk16) {
  if (const char* e = std::getenv("ZRT_POOL")) return std::atoi(e) != 0;
  return !stk16;
}
// Compressed wide nodes (wide_iter_q, MODE 8 / 9) for this tree?  ZRT_QNODES=1
// builds them (for trees of the path-pool loop's size, >= 65536 wide nodes, past the
// 16-bit stack, or any tree when forced); off by default: on the C5 mesh the pool
// over compressed nodes ran 7.17 Gray/s against 8.57 over the full nodes - each
// opened leaf's record is one more dependent fetch (DESIGN.md §3 "Compressed nodes")
bool want_qnodes(uint32_t n_wide) {
  if (const char* e = std::getenv("ZRT_QNODES")) return std::atoi(e) != 0;
  (void)n_wide;
  return false;
}
// Top levels of a compressed tree served from LDS (ZRT_QTOP overrides): every ray
// reads the root and a level-1 node, most a level-2 node - with 64-B nodes the
// third level (<= 21 nodes, 10.5 KiB of octant copies) fits beside the pool's queues
uint32_t qtop_levels() {
  if (const char* e = std::getenv("ZRT_QTOP")) return uint32_t(std::max(1, std::min(4, std::atoi(e))));
  return 3;
}
// The list loop with per-lane work items (render_loop_list, MODE 6) for scenes
// without a BVH; ZRT_LIST_LANES=0 forces the wave-unit loop (render_loop MODE 0).
// C2: 34.1 (MODE 0, lanes in per-sample lockstep) -> 45.4 (MODE 0, free lanes
// within a unit) -> MODE 6.
static bool use_list_lanes() {
  if (const char* e = std::getenv("ZRT_LIST_LANES")) return std::atoi(e) != 0;
  return true;
}
// LDS of the path-pool loop's rays, hits and queues per block (render_loop_pool)
static size_t pool_lds_bytes() { return ((8 * sizeof(float) + 1) * K.block_paths + 15) & ~size_t(15); }

// Every region of a plan inside the block's share and disjoint from the others,
// float4 regions 16-B aligned (the kernels index them from lds_raw by these
// offsets, nothing else keeps them apart); a violation is a bug in plan_lds.
static void check_plan(const LdsPlan& L) {
  struct Reg { size_t off, n; const char* name; bool f4; };
  const Reg regs[] = {{0, L.stack_b, "stack", false}, {L.top_off, L.top_b, "top nodes", true},
                      {L.pool_off, L.pool_b, "pool", true}, {L.state_off, L.state_b, "lane state", false},
                      {L.att_off, L.att_b, "attenuation rows", false}, {L.mat_off, L.mats_b, "materials", true}};
  if (L.bytes > kLdsPerBlockMax)
    throw Error(ZRT_E_UNSUPPORTED, "LDS plan: " + std::to_string(L.bytes) + " B, past a block's " +
                                       std::to_string(kLdsPerBlockMax) + " B");
  for (const Reg& x : regs) {
    if (!x.n) continue;
    if (x.off + x.n > L.bytes)
      throw Error(ZRT_E_UNSUPPORTED, std::string("LDS plan: ") + x.name + " past the plan's end");
    if (x.f4 && x.off % 16)
      throw Error(ZRT_E_UNSUPPORTED, std::string("LDS plan: ") + x.name + " not 16-B aligned");
    for (const Reg& y : regs)
      if (&x != &y && y.n && x.off < y.off + y.n && y.off < x.off + x.n)
        throw Error(ZRT_E_UNSUPPORTED, std::string("LDS plan: ") + x.name + " overlaps " + y.name);
  }
}
// tests: a cap on the FAST stack's LDS rows, so that the global overflow rows come
// into use.  ZRT_STACK_LDS_ROWS=<n> also forces the 32-bit stack (fast_stk16);
// ZRT_STACK_LDS_ROWS16=<n> caps the rows the same way and leaves the stack's width
// alone, so a 16-bit stack reads its overflow rows too.
uint32_t stack_rows_cap() {
  const char* f = std::getenv("ZRT_STACK_LDS_ROWS");
  if (!f) f = std::getenv("ZRT_STACK_LDS_ROWS16");
  return f ? uint32_t(std::atoi(f)) : kNoRowsCap;
}
// FAST: a 16-bit stack when node indices fit (either width keeps its first rows in
// LDS and deeper ones in global memory, plan_lds)
bool fast_stk16(uint32_t n_wide, uint32_t n_nodes) {
  return n_wide < 65536 && n_nodes < 65536 && !std::getenv("ZRT_STACK_LDS_ROWS");
}
// pool: the path-pool loop (MODE 5): its attenuation rows are per path
// (kBlockPaths per block), and its rays / hits / queues follow them.
// The lockstep FAST loop (mode 3, neither wf nor pool) also holds its lane state
// (LaneState) and keeps at most ZRT_STACK_ROWS_LOCK stack rows in LDS.
LdsPlan plan_lds(uint32_t n_top, uint32_t n_mats, int mode, bool stk16, uint32_t stack_depth, uint32_t max_depth,
                 bool wf, bool pool, uint32_t prng, uint32_t node_f4, uint32_t rows_cap) {
  const uint32_t waves = mode == 3 ? (pool ? K.waves_pool : wf ? K.waves_wf : K.waves_wide)
                         : mode == 0 ? K.waves_list : K.waves_per_simd;
  // 256-thread blocks: `waves` blocks per CU; 1 KiB below the even share (a
  // block of exactly 32 KiB ran 8 % slower at 5 blocks per CU)
  const size_t budget = (160u << 10) / waves - (1u << 10);
  const size_t entry = stk16 ? sizeof(uint16_t) : sizeof(uint32_t);
  const size_t row_att = sizeof(uint32_t) * (pool ? K.block_paths : kBlock);  // one att code per lane / path
  const size_t top = mode == 3 ? size_t(n_top) * node_f4 * sizeof(float4) * K.oct_copies : 0;
  const size_t pool_b = pool ? pool_lds_bytes() : 0;
  const bool lock = mode == 3 && !wf && !pool;
  const size_t state = lock ? size_t(K.lane_words[prng == ZRT_PRNG_XOSHIRO256]) * 4u * kBlock : 0;
  // attenuation rows wanted: rows 0 .. max_depth-2 are ever pushed (raytrace.zig:99 at depth > 1).
  // A row is one 4-B att code per lane (att_code; round 3: three floats, 12 B), so
  // the same LDS holds three times the rows: the lockstep loop 6 (round 3, 2 rows
  // of floats - C4 A/B: none 50.35, 1 row 50.57, 2 rows 50.70 Gray/s; a 32 KiB
  // block 46.5), the wavefront loop 12 (its 4 blocks per CU have a larger share;
  // the textured C5 mesh scatters often), the path pool 3 per path, the list loops
  // 24 (no stack, no tree in LDS; C2 at depth 30 with glass: round 3 2 -> 4 -> 8
  // rows of floats 32.7 -> 33.3 -> 34.0 Gray/s, profiles/r03/ab12)
  const uint32_t att_cap = pool ? K.att_rows_pool : wf ? K.att_rows_wf : mode == 0 ? K.att_rows_list : K.att_rows_lock;
  uint32_t want = att_cap;
  if (const char* e = std::getenv("ZRT_ATT_LDS_ROWS")) want = uint32_t(std::atoi(e));
  want = std::min<uint32_t>(want, max_depth > 1 ? max_depth - 1 : 0);
  LdsPlan L;
  L.budget = budget;
  if (mode == 3) {
    // the stack takes what the top nodes, the lane state and the wanted attenuation
    // rows leave (the lockstep loop: at most ZRT_STACK_ROWS_LOCK rows; it wants
    // ZRT_ATT_ROWS_LOCK att rows); deeper rows live in global memory (wide_iter and
    // wide_iter_q read them at either stack width, so no FAST plan holds a stack
    // the block's LDS cannot)
    want = std::min<uint32_t>(want, att_cap);
    const size_t fixed = top + pool_b + state + want * row_att;
    const size_t room = budget > fixed ? budget - fixed : 0;
    L.stack_rows = std::max<uint32_t>(1, std::min<uint32_t>(stack_depth, uint32_t(room / (kBlock * entry))));
    if (lock) L.stack_rows = std::min<uint32_t>(L.stack_rows, K.stack_rows_lock);
  } else {
    L.stack_rows = stack_depth;  // BINARY / REFERENCE: the whole stack in LDS (check_plan: within a block's LDS)
  }
  if (rows_cap != kNoRowsCap && mode == 3)  // tests: force the overflow rows into use
    L.stack_rows = std::max<uint32_t>(1, std::min<uint32_t>(L.stack_rows, rows_cap));
  const size_t stack = (size_t(L.stack_rows) * kBlock * entry + 15) & ~size_t(15);
  const size_t used = stack + top + pool_b + state;
  // loops that read the material table from LDS only (the lockstep and list loops): the table
  // before the attenuation rows, which live in global memory when LDS runs out
  const size_t mats = size_t(n_mats) * sizeof(DevMaterial);
  const bool mats_first = lock || mode == 0;
  const size_t mats_res = mats_first && used + mats <= budget ? mats : 0;
  L.att_rows = std::min<uint32_t>(want, used + mats_res < budget ? uint32_t((budget - used - mats_res) / row_att) : 0u);
  L.top_off = uint32_t(stack);
  L.pool_off = uint32_t(stack + top);
  L.state_off = uint32_t(stack + top + pool_b);
  L.att_off = uint32_t(used);
  L.bytes = used + L.att_rows * row_att;
  L.stack_b = size_t(L.stack_rows) * kBlock * entry;
  L.top_b = top;
  L.pool_b = pool_b;
  L.state_b = state;
  L.att_b = L.att_rows * row_att;
  // the material table, if it fits what is left (ZRT_MATS_LDS=0: A/B, always global,
  // for the loops that can read it there)
  const char* me = std::getenv("ZRT_MATS_LDS");
  if (mats > 0 && L.bytes + mats <= budget && (mats_first || !(me && std::atoi(me) == 0))) {
    L.mat_off = uint32_t(L.bytes);
    L.mats_in_lds = 1;
    L.bytes += mats;
    L.mats_b = mats;
  }
  // the lockstep FAST kernel's waves per SIMD hold only within the share (the
  // other loops' plans may exceed it: their launch then fits fewer blocks per CU)
  if (lock && L.bytes > budget) throw Error(ZRT_E_UNSUPPORTED, "LDS plan: the lockstep loop's regions exceed its share");
  check_plan(L);
  return L;
}

// global attenuation rows a path (a lane; the path pool: a path) is given
uint32_t att_rows_per_path(const LdsPlan& lp, uint32_t max_depth) {
  return std::max<uint32_t>(1, max_depth - std::min(max_depth, lp.att_rows));
}
BufNeed buffer_need(const LdsPlan& lp, uint32_t max_depth, uint32_t stack_depth, uint64_t n_paths, uint64_t n_lanes,
                    bool stk16) {
  BufNeed n;
  n.att_elems = uint64_t(att_rows_per_path(lp, max_depth)) * n_paths;
  if (stack_depth > lp.stack_rows)
    n.ovf_bytes = uint64_t(stack_depth - lp.stack_rows) * n_lanes * (stk16 ? sizeof(uint16_t) : sizeof(uint32_t));
  return n;
}
void check_buffers(const char* launch, const BufNeed& need, uint64_t att_elems, uint64_t ovf_bytes) {
  if (need.att_elems > att_elems)
    throw Error(ZRT_E_UNSUPPORTED, std::string(launch) + ": needs " + std::to_string(need.att_elems) +
                                       " global attenuation-row entries, the context holds " + std::to_string(att_elems));
  if (need.ovf_bytes > ovf_bytes)
    throw Error(ZRT_E_UNSUPPORTED, std::string(launch) + ": needs " + std::to_string(need.ovf_bytes) +
                                       " B of global stack rows, the context holds " + std::to_string(ovf_bytes));
}
// The device side of the same check (KArgs::att_cap / ovf_cap: the allocations'
// elements), in the STATS flavour: a row index past its buffer sets kErrBounds and
// the access is skipped (tests/test_gpu_runtime.py shrinks the capacity it is told)
uint64_t ovf_cap_elems(uint64_t ovf_bytes, bool stk16) { return ovf_bytes / (stk16 ? 2u : 4u); }

// ZRT_LEAN=0 forces the general kernel; an ineligible launch never takes the lean one
static bool lean_wanted() {
  if (const char* e = std::getenv("ZRT_LEAN")) return std::atoi(e) != 0;
  return true;
}
// KArgs::check_origins of a render launch is 0: its camera lies inside the scene's origin bound
bool camera_inside(const zrt_camera* cam, const float root_c[3], float origin_bound) {
  const float m = std::max({std::fabs(cam->origin.x - root_c[0]), std::fabs(cam->origin.y - root_c[1]),
                            std::fabs(cam->origin.z - root_c[2])});
  return m <= origin_bound;
}
// The kernel of one launch: the lean one where the plan allows it, for the timed
// flavour (the STATS flavour stays general) of a launch that checks no origin
bool lean_launch(const LaunchPlan& P, bool stats, bool cam_inside) { return P.lean && !stats && cam_inside; }
// zrt_stats::sampling_loop of a kernel: the path pool's flavours report as the pool
uint32_t reported_loop(int kmode) { return kmode == 7 || kmode == 8 || kmode == 9 ? 5u : uint32_t(kmode); }
LaunchPlan plan_launch(const SceneShape& s, const zrt_params* p) {
  LaunchPlan P;
  P.mode = !s.use_bvh ? 0 : p->traversal == ZRT_TRAVERSAL_REFERENCE ? 2 : p->traversal == ZRT_TRAVERSAL_BINARY ? 1 : 3;
  const int mode = P.mode;
  // (FAST also holds the reference traversal's rows for its order-hazard replay)
  P.stack_depth = mode == 3 ? std::max(s.wide_stack, s.stack_depth) : s.stack_depth;
  if (const char* cap = std::getenv("ZRT_DEBUG_STACK_CAP"))  // tests: a stack too small for the tree
    P.stack_depth = std::max<uint32_t>(4, std::min<uint32_t>(P.stack_depth, uint32_t(std::atoi(cap))));
  P.stk16 = mode == 3 ? fast_stk16(s.n_wide, s.n_nodes) : s.n_nodes < 65536;
  // no loop shades at max_depth 0 (every sample ends at the depth limit before it
  // traces): the lockstep / list loops return black there; the wavefront and
  // path-pool loops assume max_depth >= 1 and are never chosen
  const bool shades = p->max_depth >= 1;
  // FAST: the wavefront loop (MODE 4) where lanes' traversal lengths diverge
  P.wf = mode == 3 && shades && use_wavefront(P.stk16);
  // the grazing-triangle guard (ZRT_FLAG_GUARD): carried by the path-pool loop's traversal
  P.guard_on = mode == 3 && (p->flags & ZRT_FLAG_GUARD) != 0 && s.guard > 0.0f;
  // the path-pool loop (MODE 5) for the same cases, when asked for; a 16-bit stack
  // must fit beside its rays and queues in the block's LDS share, else the 32-bit
  // stack with overflow rows
  P.pool = mode == 3 && shades && (use_pool(P.stk16) || P.guard_on);
  // the path pool over compressed nodes (MODE 8 / 9) where the context built them
  P.qn = P.pool && s.q_ok;
  P.node_f4 = P.qn ? kQuantNodeF4 : 8u;
  const uint32_t n_top = P.qn ? s.q_top : s.n_top;
  if (P.pool && P.stk16) {
    const size_t budget = (160u << 10) / K.waves_pool - (1u << 10);
    const size_t top = size_t(n_top) * P.node_f4 * sizeof(float4) * K.oct_copies;
    // (rows the tests' cap keeps out of LDS need not fit it)
    const uint32_t rows = std::min(P.stack_depth, stack_rows_cap());
    if (size_t(rows) * kBlock * sizeof(uint16_t) + top + pool_lds_bytes() > budget) P.stk16 = false;
  }
  const bool list_lanes = mode == 0 && use_list_lanes();
  // (the guard's branch costs the path pool 0.7 % on C5, so a guarded render has a
  // kernel of its own, MODE 7; profiles/r04/r04n)
  P.kmode = P.pool ? (P.qn ? (P.guard_on ? 9 : 8) : (P.guard_on ? 7 : 5)) : P.wf ? 4 : list_lanes ? 6 : mode;
  // FAST: deep trees keep their last stack rows in global memory (rarely
  // touched) so the LDS never caps the occupancy the registers allow; the
  // other traversals keep the whole stack in LDS (plan_lds)
  P.lp = plan_lds(n_top, s.n_mats, mode, P.stk16, P.stack_depth, p->max_depth, P.wf, P.pool, p->prng, P.node_f4);
  if ((P.kmode == 3 || P.kmode == 6) && !P.lp.mats_in_lds) {
    // a material table past the loop's LDS share: the loop that reads it from global
    // memory (the wavefront loop for FAST, the wave-unit list loop; same images).
    // At max_depth 0 the lockstep loop stays (the wavefront loop would trace, and its
    // first scatter would write attenuation row 1 of a one-row buffer): it reads no
    // material there, and the launch copies no table into LDS (KArgs::n_mats = 0)
    if (P.kmode == 6) {
      P.kmode = 0;
    } else if (shades) {
      P.wf = true;
      P.kmode = 4;
    }
    P.lp = plan_lds(n_top, s.n_mats, mode, P.stk16, P.stack_depth, p->max_depth, P.wf, P.pool, p->prng, P.node_f4);
  }
  // the lean kernel: the lockstep FAST loop over full nodes, shading (it reads the
  // material table from LDS only), in a scene that has none of what it leaves out
  P.lean = P.kmode == 3 && shades && P.lp.mats_in_lds != 0 && s.tri_rcp_fast && !s.has_dielectric &&
           !s.has_image_texture && (p->flags & ZRT_FLAG_SCANLINES) == 0 && lean_wanted();
  return P;
}

// One pass of an accumulation run (zrt_ctx_accum_pass; zrt_debug_pass_plan reports
// the same): samples [done, done + n_samples) of a run capped at
// p->samples_per_pixel, as a launch of n_samples samples in pass_chunks chunks whose
// sample keys are shifted by `done`.  A sample's stream is keyed by
// ((pixel << 16) | sample) + seed * 0x9E37...; for sample + done < 65536,
// ((o << 16) | s) + done == (o << 16) | (s + done), so key_offset = done added to
// the seed term gives the pass the keys of the frame's samples done .. done + n - 1.
// The pass must start on a chunk boundary: its chunk sums are then the frame's
// chunks done / chunk .., and a ragged last chunk is the frame's last one.
int plan_pass(const zrt_params* p, uint32_t done, uint32_t n_samples, zrt_pass_plan* out) {
  const int rc = validate_params(p);
  if (rc) return rc;
  const uint32_t chunk = p->sample_chunk ? p->sample_chunk : ZRT_DEFAULT_SAMPLE_CHUNK;
  if (n_samples == 0) return fail(ZRT_E_INVALID, "a pass of 0 samples");
  if (uint64_t(done) + n_samples > p->samples_per_pixel)
    return fail(ZRT_E_INVALID, "the pass ends past the run's samples_per_pixel");
  if (done % chunk != 0)
    return fail(ZRT_E_INVALID, "the pass does not start on a sample chunk boundary (a ragged pass ends the run)");
  const uint32_t my_tiles = rank_tiles(geometry(p), p->rank, p->world_size);
  zrt_pass_plan P{};
  P.first_sample = done;
  P.pass_samples = n_samples;
  P.samples_after = done + n_samples;
  P.chunk = chunk;
  P.pass_chunks = (n_samples + chunk - 1) / chunk;
  P.last_chunk = n_samples - (P.pass_chunks - 1) * chunk;
  if (uint64_t(my_tiles) * 64u * P.pass_chunks >= (1ull << 32) - (1ull << 26))  // (+ one refill per lane of slack)
    return fail(ZRT_E_UNSUPPORTED, "more than 2^32 (pixel, chunk) work items");
  P.partial_bytes = uint64_t(my_tiles) * 64u * P.pass_chunks * sizeof(float4);
  P.key_offset = done;
  *out = P;
  return ZRT_OK;
}

// The levels of an adaptive run (zrt.h "adaptive sampling"; zrt_debug_adapt_plan
// reports the same): L_0 = first_level in whole chunks (at least one), doubled while
// below the cap, then the cap.  Every level but the last ends on a chunk boundary, so
// every level is a pass plan_pass accepts.
int plan_adapt(const zrt_params* p, const zrt_adaptive* ad, std::vector<uint32_t>* levels) {
  if (!ad) return fail(ZRT_E_INVALID, "null argument");
  zrt_pass_plan whole{};
  const int rc = plan_pass(p, 0u, p ? p->samples_per_pixel : 0u, &whole);  // (validates the params and the cap)
  if (rc) return rc;
  if (!(ad->tolerance >= 0.0f) || !std::isfinite(ad->tolerance))
    return fail(ZRT_E_INVALID, "zrt_adaptive.tolerance must be finite and >= 0");
  const uint64_t cap = p->samples_per_pixel, chunk = whole.chunk;
  uint64_t L = std::max<uint64_t>(1u, (uint64_t(ad->first_level) + chunk - 1) / chunk) * chunk;
  levels->clear();
  for (; L < cap; L *= 2) levels->push_back(uint32_t(L));
  levels->push_back(uint32_t(cap));
  return ZRT_OK;
}

// The host half of the variance plane (zrt.h "the variance plane";
// zrt_debug_variance_plan reports the same): n samples in chunks of c are k = n / c
// chunk sums; ik and sc in f32 as the header states them.  Refused: no sample, a
// ragged n (its last chunk sum is missing from Q), fewer than two chunks.
int plan_variance(const zrt_params* p, uint32_t n, zrt_variance_plan* out) {
  const int rc = validate_params(p);
  if (rc) return rc;
  const uint32_t chunk = p->sample_chunk ? p->sample_chunk : ZRT_DEFAULT_SAMPLE_CHUNK;
  if (n == 0) return fail(ZRT_E_INVALID, "variance: no samples in the accumulator");
  if (n % chunk != 0)
    return fail(ZRT_E_INVALID, "variance: " + std::to_string(n) + " samples are not whole chunks of " +
                                   std::to_string(chunk) + " (a ragged pass happened; choose a sample_chunk that "
                                   "divides the samples)");
  const uint32_t k = n / chunk;
  if (k < 2)
    return fail(ZRT_E_INVALID, "variance: " + std::to_string(n) + " samples are fewer than two chunks of " +
                                   std::to_string(chunk) + " (choose a smaller sample_chunk)");
  out->chunk = chunk;
  out->k = k;
  out->ik = 1.0f / float(k);
  out->sc = 1.0f / (float(k - 1) * (float(chunk) * float(chunk)));
  return ZRT_OK;
}

// What the filters refuse of a zrt_denoise (after their params), and the launch's settings otherwise.
static int denoise_settings(const zrt_denoise* dn, DenoiseLaunch* out) {
  if (dn->iterations > 8) return fail(ZRT_E_INVALID, "denoise iterations must be <= 8");
  const float sg[4] = {dn->sigma_color, dn->sigma_normal, dn->sigma_albedo, dn->sigma_depth};
  const char* names[4] = {"sigma_color", "sigma_normal", "sigma_albedo", "sigma_depth"};
  float inv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  uint32_t terms = 0;
  for (int k = 0; k < 4; ++k) {
    if (!std::isfinite(sg[k]) || sg[k] < 0.0f)
      return fail(ZRT_E_INVALID, std::string("denoise ") + names[k] + " must be finite and >= 0");
    if (sg[k] > 0.0f) {
      terms |= 1u << k;
      inv[k] = 1.0f / sg[k];
    }
  }
  out->iterations = dn->iterations ? dn->iterations : ZRT_DEFAULT_DENOISE_ITERATIONS;
  out->terms = terms;
  out->inv_c = inv[0];
  out->inv_n = inv[1];
  out->inv_a = inv[2];
  out->inv_z = inv[3];
  return ZRT_OK;
}

// What zrt_ctx_denoise refuses of a zrt_denoise, and the launch it asks for otherwise.
int plan_denoise(const zrt_params* p, const zrt_denoise* dn, DenoiseLaunch* out) {
  if (!dn) return fail(ZRT_E_INVALID, "denoise is null");
  int rc = validate_params(p);
  if (rc) return rc;
  rc = denoise_settings(dn, out);
  if (rc) return rc;
  out->width = p->width;
  out->n = p->height;
  return ZRT_OK;
}

// zrt_rect_check (zrt.h "denoising lens frames"): the frame as the camera query takes it - the
// whole width, height > width allowed - and a rectangle inside it.
int check_rect(const zrt_params* p, const zrt_rect* r) {
  if (!p || !r) return fail(ZRT_E_INVALID, "null argument");
  if (p->width == 0 || p->height == 0 || p->width > 65535 || p->height > 65535)
    return fail(ZRT_E_INVALID, "camera: width and height must be 1 .. 65535");
  if (p->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  if (p->prng > ZRT_PRNG_XOSHIRO256) return fail(ZRT_E_INVALID, "unknown prng");
  if (r->w == 0 || r->h == 0) return fail(ZRT_E_INVALID, "camera: the rectangle is empty");
  if (r->x0 >= p->width || r->w > p->width - r->x0 || r->y0 >= p->height || r->h > p->height - r->y0)
    return fail(ZRT_E_INVALID, "camera: the rectangle leaves the frame");
  return ZRT_OK;
}

// zrt_ctx_denoise_rect's refusals that need no context, and its launch: plan_denoise without
// raytrace.zig:168's square (l->n is not used; the rectangle is the domain).
int plan_denoise_rect(const zrt_params* p, const zrt_denoise* dn, const zrt_rect* r, DenoiseLaunch* out) {
  if (!dn) return fail(ZRT_E_INVALID, "denoise is null");
  int rc = check_rect(p, r);
  if (rc) return rc;
  rc = denoise_settings(dn, out);
  if (rc) return rc;
  out->width = p->width;
  out->n = 0;
  return ZRT_OK;
}

// zrt_ctx_camera_variance's plan: plan_variance's (k, ik, sc) and refusals of (sample_chunk,
// n_total); the frame's extents are check_rect's business (a lens frame may be taller than wide).
int plan_camera_variance(const zrt_params* p, const zrt_rect* r, uint32_t n_total, zrt_variance_plan* out) {
  int rc = check_rect(p, r);
  if (rc) return rc;
  zrt_params q = *p;
  q.width = q.height = q.samples_per_pixel = 1;
  return plan_variance(&q, n_total, out);
}

// The reprojection plan of a previous camera (zrt.h "temporal accumulation";
// zrt_debug_reproject_plan reports the same): every cross product component is one
// a*b - c*d, the dot product (x + y) + z, all f32 (this file is built unfused).
int plan_reproject(const zrt_camera* prev, const zrt_params* p, zrt_reproject_plan* out) {
  if (!prev) return fail(ZRT_E_INVALID, "null argument");
  const int rc = validate_params(p);
  if (rc) return rc;
  const zrt_vec3 o = prev->origin, H = prev->horizontal, W = prev->vertical;
  const zrt_vec3 b = {prev->lower_left_corner.x - o.x, prev->lower_left_corner.y - o.y,
                      prev->lower_left_corner.z - o.z};
  const auto cross = [](const zrt_vec3& a, const zrt_vec3& c) {
    return zrt_vec3{a.y * c.z - a.z * c.y, a.z * c.x - a.x * c.z, a.x * c.y - a.y * c.x};
  };
  zrt_vec3 rn = cross(W, H), ru = cross(b, W), rv = cross(H, b);
  const float s = (b.x * rn.x + b.y * rn.y) + b.z * rn.z;
  if (s < 0.0f) {
    rn = zrt_vec3{-rn.x, -rn.y, -rn.z};
    ru = zrt_vec3{-ru.x, -ru.y, -ru.z};
    rv = zrt_vec3{-rv.x, -rv.y, -rv.z};
  }
  out->origin = o;
  out->rn = rn;
  out->ru = ru;
  out->rv = rv;
  out->s = s;
  out->valid = (s < 0.0f || s > 0.0f) ? 1u : 0u;  // (0 and NaN: no)
  return ZRT_OK;
}

// What zrt_ctx_temporal refuses of a zrt_temporal, and the camera-independent part
// of the launch it asks for otherwise.
int plan_temporal(const zrt_params* p, const zrt_temporal* tp, TemporalLaunch* out) {
  if (!tp) return fail(ZRT_E_INVALID, "temporal is null");
  const int rc = validate_params(p);
  if (rc) return rc;
  if (!(tp->alpha_min >= 0.0f && tp->alpha_min <= 1.0f))
    return fail(ZRT_E_INVALID, "temporal alpha_min must lie in [0, 1]");
  if (tp->max_history > 65535u) return fail(ZRT_E_INVALID, "temporal max_history must be <= 65535");
  if (tp->flags & ~uint32_t(ZRT_TA_DEMODULATE)) return fail(ZRT_E_INVALID, "temporal: unknown flag");
  const float sg[2] = {tp->sigma_normal, tp->sigma_depth};
  const char* names[2] = {"sigma_normal", "sigma_depth"};
  const uint32_t bit[2] = {kDnNormal, kDnDepth};
  float inv[2] = {0.0f, 0.0f};
  uint32_t terms = 0;
  for (int k = 0; k < 2; ++k) {
    if (!std::isfinite(sg[k]) || sg[k] < 0.0f)
      return fail(ZRT_E_INVALID, std::string("temporal ") + names[k] + " must be finite and >= 0");
    if (sg[k] > 0.0f) {
      terms |= bit[k];
      inv[k] = 1.0f / sg[k];
    }
  }
  *out = TemporalLaunch{};
  out->width = p->width;
  out->n = p->height;
  out->terms = terms;
  out->demod = (tp->flags & ZRT_TA_DEMODULATE) ? 1u : 0u;
  out->max_history = tp->max_history ? tp->max_history : uint32_t(ZRT_DEFAULT_TEMPORAL_HISTORY);
  out->alpha_min = tp->alpha_min;
  out->inv_n = inv[0];
  out->inv_z = inv[1];
  out->f_width = float(p->width);
  out->f_height = float(p->height);
  return ZRT_OK;
}
}  // namespace zrt

int zrt_rect_check(const zrt_params* params, const zrt_rect* rect) { return zrt::check_rect(params, rect); }
