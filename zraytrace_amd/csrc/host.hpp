// host.hpp - the host side that needs no device: validation and tile geometry,
// the LDS / buffer / launch / pass planners (planner.cpp) and the scene flattened
// for upload (flatten.cpp).  No HIP runtime call is made behind this header; HIP
// supplies the float4 type only.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <functional>
#include <new>
#include <vector>

#include "denoise.hpp"
#include "kernels.hpp"
#include "temporal.hpp"
#include "zrt.hpp"

namespace zrt {
struct Geometry {
  uint32_t xbound, tiles_x, tiles_y, n_tiles;
};

// The scene flattened for the device (host arrays, built once, uploaded to
// every GPU that renders it).
struct HostScene {
  bool use_bvh = false;
  uint32_t n_prims = 0, n_nodes = 0, bvh_depth = 0;
  uint32_t n_wide = 0, n_leaves = 0, wide_stack = 0, wide_stride = 0, n_top = 0, n_mats = 0;
  uint32_t texel_bytes = 0;
  uint32_t tri_rcp_fast = 1;  // KArgs::tri_rcp_fast
  // a dielectric / an image-textured material in the table (used or not): no lean kernel (plan_launch)
  uint32_t has_dielectric = 0, has_image_texture = 0;
  float scene_extent = 0.0f;  // KArgs::scene_extent
  float tri_c[3] = {0.0f, 0.0f, 0.0f}, tri_h[3] = {0.0f, 0.0f, 0.0f};  // KArgs::tri_c / tri_h
  float root_c[3] = {0.0f, 0.0f, 0.0f}, origin_bound = 0.0f;  // KArgs::root_c / origin_bound
  uint32_t layout = 0;           // KArgs::layout: the wide tree's encoding
  float graze_m = 0x1p-18f;      // KArgs::graze_m (the inner boxes are grown by half of it)
  float graze_leaf = 0x1p-18f;   // KArgs::graze_leaf
  float guard = 0.0f;            // KArgs::guard
  std::vector<uint8_t> ref_sph;  // KArgs::ref_sph
  std::vector<float4> nodes, wn, prims, shade;
  std::vector<float4> qn, ql;  // compressed wide nodes (8 octant copies) and leaf records, when q_ok
  bool q_ok = false;
  uint32_t q_stride = 0;       // float4s per octant copy of qn
  uint32_t q_top = 0;          // compressed nodes served from LDS (their top levels)
  std::vector<DevMaterial> mats;
  std::vector<float> tex;
  std::vector<uint32_t> tex8;
  std::vector<uint32_t> slot_to_prim;  // device primitive slot -> reference list index
  std::vector<uint32_t> leaf_of_slot;  // device primitive slot -> its reference BVH leaf node
  double preprocess_ms = 0;
  bool device_bvh_failed = false;  // the device BVH build threw (the caller clears HIP's sticky error)
};

// The block's dynamic LDS: [stack rows][lane] (StackT), then (FAST) the top
// wide nodes of every octant copy, then the first attenuation rows
// [row][rgb][lane] f32.  Sized so the waves per SIMD the kernel is built for
// (its __launch_bounds__) still fit: 160 KiB / that many blocks per CU.
struct LdsPlan {
  uint32_t stack_rows = 0, top_off = 0, att_off = 0, att_rows = 0, mat_off = 0, mats_in_lds = 0, pool_off = 0;
  uint32_t state_off = 0;
  size_t bytes = 0, budget = 0;
  size_t stack_b = 0, top_b = 0, pool_b = 0, state_b = 0, att_b = 0, mats_b = 0;  // region sizes (check_plan)
};
constexpr size_t kLdsPerBlockMax = 160u << 10;  // gfx950: a work-group may use the CU's whole LDS

// The context's global buffers that the launches of a frame share (the render
// launch and its scheduling probe) and that later frames reuse: attenuation rows
// past the plan's LDS rows ([row][lane], the path pool [row][path]: elements of
// c->att) and FAST stack rows past the plan's LDS rows ([row][lane]: bytes of
// c->stack_ovf).  A launch's need follows from its own plan; every launch is
// checked against the allocation before it is enqueued (check_buffers), so a
// sizing mistake - round 5's scheduling probe kept 4 LDS attenuation rows where
// the wavefront render it shared the buffer with kept 12 - is refused as
// ZRT_E_UNSUPPORTED on the host instead of faulting on the GPU.
struct BufNeed {
  uint64_t att_elems = 0;  // u32 attenuation codes
  uint64_t ovf_bytes = 0;  // stack entries (StackT) past the LDS rows
};

// What the launch decision reads of a flattened scene (shape_of): a context keeps
// it with its upload, zrt_debug_launch_plan takes it with no device.
struct SceneShape {
  bool use_bvh = false, q_ok = false;
  uint32_t n_nodes = 0, n_wide = 0, wide_stack = 0, stack_depth = 0, n_top = 0, q_top = 0, n_mats = 0;
  float guard = 0.0f;
  bool tri_rcp_fast = false, has_dielectric = true, has_image_texture = true;  // (the lean kernel's conditions)
};

// The launch decision of a render (zrt_ctx_render_tiles; zrt_debug_launch_plan
// reports it with no device): traversal mode, stack width and depth, sampling
// loop (kmode: the kernel's MODE), node format and the block's LDS plan.  Pure:
// it reads the scene's shape, the params and the environment knobs only.
struct LaunchPlan {
  int mode = 0;   // 0 list, 1 binary, 2 reference, 3 FAST
  int kmode = 0;  // the kernel: mode, or 4 wavefront, 5 / 7 / 8 / 9 path pool, 6 list with per-lane items
  bool stk16 = false, wf = false, pool = false, qn = false, guard_on = false;
  // the timed launch may take the lean kernel (render.hip struct Lean): the scene and the params
  // allow it; the launch itself adds that its camera lies inside the origin bound
  // and that it is not the STATS flavour (lean_launch)
  bool lean = false;
  uint32_t node_f4 = 8, stack_depth = 0;
  LdsPlan lp;
};

// ---- planner.cpp ----
double now_ms();
int validate_scene(const zrt_scene* s);
int validate_params(const zrt_params* p);
Geometry geometry(const zrt_params* p);
uint32_t rank_tiles(const Geometry& g, uint32_t rank, uint32_t world);
// A rank's tiles in local order: f(local tile, in-frame width, in-frame height, first row).
void for_rank_tiles(const Geometry& g, uint32_t height, uint32_t rank, uint32_t world,
                    const std::function<void(uint32_t lt, uint32_t w, uint32_t h, uint32_t y0)>& f);
float paxis_threshold();
void check_octant_offsets(uint32_t stride_f4, uint32_t n_top, uint32_t node_f4);
bool want_qnodes(uint32_t n_wide);
uint32_t qtop_levels();
constexpr uint32_t kNoRowsCap = 0xffffffffu;
uint32_t stack_rows_cap();
bool fast_stk16(uint32_t n_wide, uint32_t n_nodes);
LdsPlan plan_lds(uint32_t n_top, uint32_t n_mats, int mode, bool stk16, uint32_t stack_depth, uint32_t max_depth,
                 bool wf, bool pool, uint32_t prng, uint32_t node_f4 = 8, uint32_t rows_cap = stack_rows_cap());
uint32_t att_rows_per_path(const LdsPlan& lp, uint32_t max_depth);
BufNeed buffer_need(const LdsPlan& lp, uint32_t max_depth, uint32_t stack_depth, uint64_t n_paths, uint64_t n_lanes,
                    bool stk16);
void check_buffers(const char* launch, const BufNeed& need, uint64_t att_elems, uint64_t ovf_bytes);
uint64_t ovf_cap_elems(uint64_t ovf_bytes, bool stk16);
bool camera_inside(const zrt_camera* cam, const float root_c[3], float origin_bound);
bool lean_launch(const LaunchPlan& P, bool stats, bool cam_inside);
uint32_t reported_loop(int kmode);
LaunchPlan plan_launch(const SceneShape& s, const zrt_params* p);
int plan_pass(const zrt_params* p, uint32_t done, uint32_t n_samples, zrt_pass_plan* out);
int plan_adapt(const zrt_params* p, const zrt_adaptive* ad, std::vector<uint32_t>* levels);
int plan_variance(const zrt_params* p, uint32_t n, zrt_variance_plan* out);
int plan_denoise(const zrt_params* p, const zrt_denoise* dn, DenoiseLaunch* out);
int check_rect(const zrt_params* p, const zrt_rect* r);
int plan_denoise_rect(const zrt_params* p, const zrt_denoise* dn, const zrt_rect* r, DenoiseLaunch* out);
int plan_camera_variance(const zrt_params* p, const zrt_rect* r, uint32_t n_total, zrt_variance_plan* out);
int plan_reproject(const zrt_camera* prev, const zrt_params* p, zrt_reproject_plan* out);
int plan_temporal(const zrt_params* p, const zrt_temporal* tp, TemporalLaunch* out);

// ---- radiance.cpp (its part that needs no device) ----
// zrt_ctx_radiance's refusals of params, rq and n, and its launch (zrt_debug_radiance_plan).
int plan_radiance(const zrt_params* p, const struct zrt_radiance* rq, uint32_t n, uint32_t cu_count, uint64_t partial_cap,
                  zrt_radiance_plan* out);

// ---- camera_query.cpp (its part that needs no device) ----
// zrt_ctx_camera's refusals of params and the query, and its launch: the slots of the
// rectangle and plan_radiance over them (zrt_debug_camera_plan); its refusals of the lens.
int plan_camera(const zrt_params* p, const zrt_camera_query* cq, uint32_t cu_count, uint64_t partial_cap,
                zrt_camera_plan* out);
int check_lens(const zrt_lens* lens);

// ---- tile_class.cpp: the all-sky tiles of a frame (DESIGN.md §3 "All-sky tiles") ----
// A tile's class word: bit 31 (kTileFrozen's bit, so compact_kernel drops such tiles
// from a tile order) marks a tile no primary ray of which can hit anything; the low
// bits are free for later classes.
constexpr uint32_t kTileGeneral = 0u, kTileSky = kTileFrozen;
// One-sphere tiles (DESIGN.md §3 "One-sphere tiles"): bit 30, with the device slot of the
// one sphere a primary ray of the tile can hit in the low bits.
constexpr uint32_t kTileOneSphere = 0x40000000u;
struct SkyNode {  // a reference-tree node: its box's bounding sphere and its children (KArgs::nodes refs)
  double c[3], r;
  int32_t left, right;
};
struct SkyPrim {  // a primitive slot's bounding sphere; sphere_index >= 0: a sphere (r: its radius)
  double c[3], r;
  int32_t sphere_index;
};
struct SphereArgs {  // a sphere's reference leaf box and its record {center.xyz, radius^2} (KArgs::one_*)
  float lo[3], hi[3], rec[4];
};
// What the classifier keeps of a flattened scene (a context keeps it past the upload).
struct SkyScene {
  bool ok = false;  // false: every tile is general (no tree, a non-finite plane, a tree too large to keep)
  bool has_tri = false;
  std::vector<SkyNode> nodes;
  std::vector<SkyPrim> prims;
  std::vector<uint32_t> spheres;  // the slots that hold spheres
  double k_ao = 0, k_c = 0;       // the triangles' reach k_ao |ao| + k_c (tools/tri_reach_bound.py, doubled)
  double tri_c[3] = {0, 0, 0}, tri_r = 0;  // the triangles' bounding sphere
  // per sphere (`spheres` order): its reference leaf is a slot of the root wide node (the
  // one-sphere path may stand in for its traversal), and what that path reads of it
  std::vector<uint8_t> sphere_root;
  std::vector<SphereArgs> sphere_args;
};
// classify_tiles' one-sphere class: want (in): mark it; n_tiles, sphere (out): the tiles
// marked and their sphere's index in SkyScene::spheres (-1: none)
struct OneSphere {
  bool want = false;
  uint32_t n_tiles = 0;
  int32_t sphere = -1;
};
bool sky_tiles_wanted();     // ZRT_SKY_TILES (default on)
bool sphere_tiles_wanted();  // ZRT_SPHERE_TILES (default on)
bool sky_split_allowed(const LaunchPlan& P, const zrt_params* p, bool cam_inside);
bool sphere_split_allowed(const LaunchPlan& P, const zrt_params* p, bool cam_inside);
void build_sky_scene(SkyScene* s, const HostScene& h);
void classify_tiles(const SkyScene& s, const zrt_camera* cam, const zrt_params* p, std::vector<uint32_t>* cls,
                    uint32_t* n_sky, double* margins = nullptr, OneSphere* one = nullptr);

// ---- flatten.cpp ----
// `device` >= 0: the GPU that may build the reference BVH (bvh_gpu.hip); a failed
// device build falls back to the host's and sets c->device_bvh_failed
void flatten_scene(HostScene* c, const zrt_scene* s, bool use_bvh, int device, int qnodes = -1);
SceneShape shape_of(const HostScene& h);
}  // namespace zrt

// The catch clauses of the entry points that touch no device: no exception crosses the ABI.
#define ZRT_CATCH_HOST                                 \
  catch (const ::zrt::Error& e) {                      \
    return ::zrt::fail(e.code, e.what());              \
  }                                                    \
  catch (const std::bad_alloc&) {                      \
    return ::zrt::fail(ZRT_E_NOMEM, "OutOfMemory");    \
  }
