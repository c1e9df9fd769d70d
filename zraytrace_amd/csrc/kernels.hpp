// kernels.hpp - what render.hip (the kernels) and the host files share: the
// kernels' argument layout, the counter slots, the values the kernels were built
// with (KernelConfig) and the functions that name a kernel.  Plain C++: host
// files include it with hip_runtime_api.h alone.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace zrt {
// ---------------------------------------------------------------------------
// device data layout
// ---------------------------------------------------------------------------
// nodes: 2 x float4 per node {min.xyz, left}, {max.xyz, right}; child >= 0 is
//   a node index, child < 0 a primitive slot ref -(2*slot + kind) - 1.
// prims: 3 x float4 per slot (slots in DFS leaf order, or list order):
//   triangle {a.xyz, e1.x} {e1.yz, e2.xy} {e2.z, n.xyz}  (n = e1 x e2)
//   sphere   {center.xyz, radius^2} {0} {0}   (radius * radius rounded once, on the host)
// shade: 1 x float4 per slot: triangle {unit normal.xyz, tag},
//   sphere {1/radius, 0, 0, tag}; tag = material | kind << 31 (as u32 bits)
struct alignas(16) DevMaterial {
  float r, g, b, ior;          // texture color / index of refraction
  float u_off, v_off;          // image texture offsets
  uint32_t kind, tex_kind;     // ZRT_MAT_*, ZRT_TEX_*
  uint32_t img_w, img_h, img_off;  // image texture (img_off in texels of its store)
  uint32_t img_u8;                 // 1: the image is stored as 8-bit RGBX (exact k/255), 0: f32 RGB
};

struct KArgs {
  const float4* __restrict__ nodes;
  const float4* __restrict__ prims;
  const float4* __restrict__ shade;
  const float4* __restrict__ wnodes;   // FAST: 4-wide nodes (node_f4 float4 each: 8 full, 4 compressed)
  const float4* __restrict__ qleaves;  // compressed nodes' leaf records (kLeafRecF4 float4 each), else null
  uint32_t n_qnodes, n_qleaves;        // compressed nodes per octant copy and leaf records (bounds checks)
  const DevMaterial* __restrict__ mats;
  const float* __restrict__ texels;    // f32 RGB images
  const uint32_t* __restrict__ texels8;  // 8-bit RGBX images (every value exactly k/255)
  uint32_t* __restrict__ att;          // [row - att_lds_rows][lane or path]: attenuation codes (att_code)
  float4* __restrict__ partial;        // [chunk][tile slot] chunk sums
  uint32_t* __restrict__ work_counter;
  uint32_t* __restrict__ unit_cost;         // probe: loop iterations a wave spent on each tile, else null
  // lockstep render after a scheduling probe: the probe's counters, from which every
  // wave derives the same lockstep interval (render_loop, auto_sync); null: a.sync
  const unsigned long long* __restrict__ sync_probe;
  const uint32_t* __restrict__ tile_order;  // local tiles in the order units are handed out, or null
  unsigned long long* __restrict__ wave_times;  // ZRT_PROFILE builds: {start, end} realtime per wave
  unsigned long long* __restrict__ counters;  // kNumCounters x u64
  // ZRT_FLAG_SCANLINES: [row][3] recursion-limit hits, reflections, background
  // hits per frame row (raytrace.zig:184's printProgress deltas), else null
  unsigned long long* __restrict__ scanlines;
  uint32_t* __restrict__ error_flag;
  float org[3], llc[3], hor[3], ver[3];
  // jitter (raytrace.zig:173-174) divides by width / height: (x + r - 0.5) lies
  // in {+0} u [2^-23, 65536], so dev::div_core with inv_* = RN(1 / width) (IEEE on
  // the host) is the IEEE quotient with no range check
  float f_width, f_height, color_scale, inv_width, inv_height;
  uint32_t width, height, xbound, spp, max_depth;
  uint32_t tiles_x, rank, world, total_work;
  uint32_t n_list, stack_depth, n_lanes;
  uint32_t chunk, n_chunks, sync;  // a work unit = one chunk of one tile
  uint32_t n_slots;  // this launch's pixel slots (tiles x 64): the stride of a chunk in partial
  uint32_t wide_stride;  // float4s per octant copy of the wide tree
  uint32_t node_f4;      // float4s per wide node: 8 (full, wide_iter) or 4 (compressed, wide_iter_q)
  uint32_t lds_rows;     // FAST: stack rows in LDS; rows lds_rows.. stack_depth-1 in stack_ovf
  uint32_t ref_stack;    // rows the reference traversal needs (FAST's order-hazard replay)
  const uint32_t* __restrict__ leaf_of_slot;  // primitive slot -> its reference BVH leaf node
  void* stack_ovf;       // [row - lds_rows][lane] overflow rows of the FAST stack (StackT)
  unsigned long long seed_mix;
  // LDS beyond the stack rows (byte offsets into the block's dynamic LDS):
  uint32_t n_top;         // FAST: wide nodes 0 .. n_top-1 (the top levels) served from LDS
  uint32_t lds_top_off;   //   [copy][node][8] float4, copied in at kernel start
  uint32_t lds_att_off;   // attenuation rows 0 .. att_lds_rows-1: [row][lane] u32 codes (att_code)
  uint32_t att_lds_rows;  //   (rows att_lds_rows.. in `att`, [row - att_lds_rows][lane])
  uint32_t lds_mat_off;   // the material table (n_mats DevMaterial), when mats_in_lds
  uint32_t n_mats, mats_in_lds;
  uint32_t wf_thresh;  // wavefront loop: shade when ready lanes >= this / 64 of the unit's active lanes
                       // (path-pool loop: once the queue is empty and fewer than 64 - this lanes traverse)
  uint32_t lds_pool_off;  // path-pool loop: rays, hits and queues (kBlockPaths paths per block)
  uint32_t lds_state_off;  // lockstep FAST loop: lane state across the traversal, [word][lane] u32 (LaneState)
  uint32_t n_paths;       //   paths of the launch (grid x kBlockPaths): the stride of its global attenuation rows
  uint32_t tri_rcp_fast;  // every triangle |n| < 2^125: 1/det by dev::rcp_core (RayT::rcp_det)
  float scene_extent;     // the triangles' largest |coordinate| (ray_slack)
  float tri_c[3], tri_h[3];  // the triangles' bounding box: centre, half extents (paxis_grow)
  float paxis_m;             // per-axis margins in waves with a lane of max_k |1/d_k| above this (kPaxisM)
  // Spheres (DESIGN.md §3 "Spheres"): the reference BVH nodes whose subtree holds
  // a sphere (1 byte each), and the origins the wide tree's sphere growth was
  // sized for: max_k |o_k - root_c[k]| <= origin_bound (other rays are traced the
  // reference's way, ray_origin_ok)
  const uint8_t* __restrict__ ref_sph;
  float root_c[3], origin_bound;
  uint32_t check_origins;  // 0: every ray of the launch starts inside the bound (the camera does, checked
                           // on the host, and scattered rays start at hits), so ray_origin_ok is skipped
  uint32_t layout;         // the wide tree's encoding (accel_build.hpp kLayout*): must equal kKernelLayout
  float graze_m;           // the grazing margins' coefficient (RayT::gm; DESIGN.md §3 "Grazing rays")
  float graze_leaf;        // (no kernel reads it: leaf slots share graze_m; the host still fills it)
  float guard;             // the grazing-triangle guard (RayT::gk, wide_iter; 0: off)
  uint64_t att_cap, ovf_cap;  // elements of `att` and of `stack_ovf` (StackT): row_ok's bounds
  // The one-sphere kernels alone (render_loop ONE_SPHERE; DESIGN.md §3 "One-sphere tiles"):
  // the one sphere a camera ray of the launch's tiles can hit - its reference leaf's box,
  // its record {center.xyz, radius^2} and its primitive slot.  (Last, so that every other
  // field keeps its offset: the other kernels' code changes in nothing but the kernarg
  // offsets of what follows KArgs in their argument lists, hidden arguments included.)
  float one_lo[3], one_hi[3], one_rec[4];
  uint32_t one_slot;
};

// ao_kernel / ao_finish_kernel's own arguments (zrt_ctx_ao; zrt::plan_ao fills the counts)
struct AoArgs {
  uint64_t n_slots;   // pixel slots: tiles over the whole width x 64
  uint64_t n_groups;  // groups of kBlock rays (rays = n_slots x n_samples)
  uint32_t n_samples, first_sample;
  uint32_t accumulate;  // ZRT_AO_ACCUMULATE
  uint32_t in_wave;     // n_samples divides 64: the reduction ends in the wave (ZRT_AO_REDUCE_WAVE)
  uint32_t tiles_w;     // tiles over the whole width
  uint32_t rotate;      // blocks by which the groups of a round are shifted against the round before
  float radius;
};

// radiance_kernel's own arguments for one round (zrt_ctx_radiance; zrt::plan_radiance fills the counts)
struct RadianceArgs {
  uint64_t n_items;     // the round's items: n x its chunks; item k is ray k % n of the round's chunk k / n
  uint64_t key_offset;  // (first_ray << 16) + seed * 0x9E3779B97F4A7C15: key = ((ray << 16) | sample) + key_offset
  uint32_t n;           // rays
  uint32_t chunk;       // samples per chunk
  uint32_t sample0;     // the first sample of the round's chunk 0
  uint32_t sample_end;  // first_sample + n_samples of the call (the last chunk may be ragged)
};

// camera_kernel / camera_finish_kernel's own arguments for one round (zrt_ctx_camera; zrt::plan_camera fills the
// counts).  Passed by value: every field is a kernel argument, so the lens model reads scalars.
struct CameraArgs {
  uint64_t n_items;     // the round's items: n x its chunks; item k is slot k % n of the round's chunk k / n
  uint64_t key_offset;  // seed * 0x9E3779B97F4A7C15: key = ((R << 16) | sample) + key_offset, R = y * width + x
  uint32_t n;           // slots: tiles_w x tiles_h x 64 (a multiple of 64: a wave's items are one tile of one chunk)
  uint32_t chunk;       // samples per chunk
  uint32_t sample0;     // the first sample of the round's chunk 0
  uint32_t sample_end;  // first_sample + n_samples of the call (the last chunk may be ragged)
  uint32_t x0, y0, w, h;  // the rectangle; slot t * 64 + l is pixel (x0 + 8 (t % tiles_w) + (l & 7), y0 + 8 (t / tiles_w) + (l >> 3))
  uint32_t tiles_w;
  uint32_t width;       // of the frame
  uint32_t kind;        // ZRT_LENS_*
  float f_width, f_height, half_fov;
  float org[3], llc[3], hor[3], ver[3], au[3], av[3], aw[3];  // zrt_lens
};

// error_flag bits (zrt_ctx_sync / zrt_ctx_stats / zrt_render report them as ZRT_E_UNSUPPORTED)
constexpr uint32_t kErrOverflow = 1u;  // a traversal stack deeper than it was sized for
constexpr uint32_t kErrLayout = 2u;    // the wide tree's encoding is not the one this kernel decodes
constexpr uint32_t kErrBounds = 4u;    // STATS flavour: a global row index past its buffer (row_ok)

// counters[]: progress counters of raytrace.zig:20-34 + traffic diagnostics
// (kSphereTests: the one-sphere kernels count one per short-path camera ray, before the leaf
// box's loose test: also for the rays that box rejects, the sky rays of a horizon tile)
enum { kDepthHits, kReflections, kBackground, kRays, kNodes, kTriTests, kSphereTests, kShades, kTexels,
       kLeaves, kReplays, kExcessTri, kExcessSph, kExcessHits, kNumCounters };
constexpr int kWorkSlot = 14, kErrorSlot = 15, kProfSlot = 16, kScratchSlots = 48;
// STATS flavour, SIMD efficiency (zrt_ctx_debug_counters): traversal loop trips
// of the waves (per traced step, the most node visits of any lane: kNodes /
// (64 kTravTrips) is the lane efficiency of traversal), loop iterations in which
// some lane ran a rayColor step, and the lane-steps run in them
constexpr int kTravTrips = 21, kLoopTrips = 22, kLaneSteps = 23;
// STATS flavour, coherence of the FAST loop's vector-memory fetches (lane
// counts): wide nodes read from global memory, and those read while every
// active lane of the wave read the same node; primitive tests, and those in
// which every active lane tested the same primitive (a wave-uniform address
// could come through the scalar cache instead of the vector data return)
constexpr int kGlobalNodes = 24, kUniformNodes = 25, kPrimLaneTests = 26, kUniformPrims = 27;
// STATS: attenuation-stack rows written to / read from global memory (rows past
// the LDS ones): with the chunk sums, the loop's HBM writes
constexpr int kAttWrites = 28, kAttReads = 29;
// STATS: FAST traversal stack entries written to the global rows (deep trees:
// rows past the LDS ones, 32-bit entries)
constexpr int kStackOvfWrites = 30;
// scheduling probe: the loop iterations in which some lane of the wave ran a
// rayColor step, summed over the waves (with kReflections, kBackground and
// kDepthHits, the steps run: the probe's lane efficiency, auto_sync)
constexpr int kProbeTrips = 31;
// STATS: the FAST loops' vector-memory wave-instructions by shape (wave-level
// event counts, not lane counts): the inputs of bench.py's data-return model
// (DESIGN.md §4 "The data-return model"), priced per shape by
// tools/ubench_shapes.hip.  Wave trips that read a global wide node through the
// vector path (8 dwordx4 loads but for the last: 7) and the distinct nodes they
// read; trips that read one through the scalar cache; leaf trips that read a
// node's second refs (one flat dwordx4); wave trips of vector primitive tests and
// their distinct primitives; scalar primitive tests; shade records read through
// the vector path; attenuation rows written to / read from global memory.
// kVNodeCost / kVPrimCost: the same trips' sum of max(16, distinct records) - the
// data-return cycles of one of their dwordx4 loads (ubench_shapes: 16 per
// wave-instruction up to 16 distinct 64-B lines, one per line beyond)
constexpr int kVNodeTrips = 32, kVNodeLines = 33, kSNodeTrips = 34, kRbTrips = 35, kVPrimTrips = 36,
              kVPrimLines = 37, kSPrimTrips = 38, kVShadeTrips = 39, kAttWTrips = 40, kAttRTrips = 41,
              kVNodeCost = 42, kVPrimCost = 43;

// zrt_ctx_debug_counters: the tiles the last launch rendered in sky_kernel (filled in on the host)
constexpr int kSkyTilesSlot = 47;
// ... and the tiles it rendered in the one-sphere kernel (render_kernel's ONE_SPHERE instantiation)
constexpr int kSphereTilesSlot = 46;
// radiance_kernel (the query's own counters): the most attenuation rows any path of the call pushed
constexpr int kRqDeepestSlot = 44;

constexpr int kBlock = 256;
// accumulate_kernel / resolve_kernel's metrics: kMetricShards shards, kMetricStride words apart (render.hip)
constexpr uint32_t kMetricShards = 64, kMetricStride = 16, kMetricWords = kMetricShards * kMetricStride;
constexpr uint32_t kTileFrozen = 0x80000000u;  // tile_done[lt]: bit 31 set once the tile is frozen (resolve_kernel)

// The values render.hip's kernels were compiled with, which the host plans
// against (planner.cpp, flatten.cpp): the numeric ZRT_* build knobs of render.hip
// (launch sizes), the sizes that follow from them, and whether this is a profiling
// build.  Host files read this struct and no build macro,
// so a variant build (tools/variants.sh: -D flags on render.hip alone) plans for
// the kernels it really holds.
struct KernelConfig {
  uint32_t waves_wide, waves_wf, waves_pool, waves_list, waves_per_simd;  // ZRT_WAVES_*: blocks per CU of each loop
  uint32_t att_rows_lock, att_rows_wf, att_rows_pool, att_rows_list;      // ZRT_ATT_ROWS_*
  uint32_t stack_rows_lock, sync_samples, probe_spp;  // ZRT_STACK_ROWS_LOCK, ZRT_SYNC_SAMPLES, ZRT_PROBE_SPP
  uint32_t oct_copies;                                // kOctCopies: 8, the wide tree once per ray octant
  uint32_t lane_words[2];                             // LaneState<prng>::kWords
  uint32_t block_paths;                               // kBlockPaths: the path pool's paths per block
  uint32_t layout;                                    // kKernelLayout
  float paxis_m;                                      // kPaxisM
  bool profile;                                       // ZRT_PROFILE
};
const KernelConfig& kernel_config();

// The kernel of a launch (hipLaunchKernel takes it).  select_kernel: render_kernel<kmode, prng,
// stats, stack width, lean>; the others by traversal mode (8: FAST over compressed nodes).
void* select_kernel(int kmode, uint32_t prng, bool stats, bool stk16, bool lean);
// render_kernel<3, prng, stats, stack width, !stats, true>: the lockstep FAST loop whose camera
// rays test one sphere alone (tile_class.cpp proves the tiles), lean when timed, general under STATS
void* one_sphere_kernel(uint32_t prng, bool stats, bool stk16);
// compact_kernel's scheme with another predicate: the tiles of `in` whose class word equals `word`
hipError_t launch_compact_class(hipStream_t st, const uint32_t* in, uint32_t n, const uint32_t* cls, uint32_t word,
                                uint32_t* out, uint32_t* count);
void* probe_kernel(uint32_t prng, bool stk16);
void* sky_kernel_ptr(uint32_t prng, bool stats);  // the all-sky tiles' kernel (tile_class.cpp proves them)
void* trace_kernel_ptr(int mode, bool stk16);
void* features_kernel_ptr(int mode, bool stk16);
// anyhit_kernel<mode, stack width> (zrt_ctx_occluded): 0 list, 1 BINARY, 2 REFERENCE, 3 FAST over the
// full 128-B wide nodes - any-hit has no flavour over the compressed nodes
void* anyhit_kernel_ptr(int mode, bool stk16);
// ao_kernel<mode, prng, stack width> (zrt_ctx_ao): anyhit_kernel's modes
void* ao_kernel_ptr(int mode, uint32_t prng, bool stk16);
// radiance_kernel<mode, prng, stack width> (zrt_ctx_radiance): anyhit_kernel's modes
void* radiance_kernel_ptr(int mode, uint32_t prng, bool stk16);
// camera_kernel<mode, prng, stack width> (zrt_ctx_camera): radiance_kernel's modes
void* camera_kernel_ptr(int mode, uint32_t prng, bool stk16);

// One launch function per small kernel (the arguments are the kernel's, render.hip).
hipError_t launch_finalize(hipStream_t st, const float4* partial, float* out, uint32_t n_slots, uint32_t n_chunks,
                           uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound, uint32_t height,
                           float color_scale, const unsigned long long* error_flag);
hipError_t launch_accumulate(hipStream_t st, const float4* partial, float4* accum, float* out, uint32_t n_slots,
                             uint32_t pass_chunks, uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound,
                             uint32_t height, float prev_scale, float new_scale, uint32_t q_chunks,
                             const unsigned long long* error_flag, unsigned long long* metrics);
hipError_t launch_resolve(hipStream_t st, const float4* partial, float4* accum, float* out, const uint32_t* active,
                          uint32_t n_active, uint32_t my_tiles, uint32_t pass_chunks, uint32_t world, uint32_t rank,
                          uint32_t tiles_x, uint32_t xbound, uint32_t height, float prev_scale, float new_scale,
                          uint32_t q_chunks, float tolerance, uint32_t decide, uint32_t level_samples,
                          uint32_t* tile_done, const unsigned long long* error_flag, unsigned long long* metrics);
hipError_t launch_compact(hipStream_t st, const uint32_t* in, uint32_t n, const uint32_t* tile_done, uint32_t* out,
                          uint32_t* count);
hipError_t launch_assemble(hipStream_t st, const float* gathered, float* frame, const uint32_t* rank_base,
                           uint32_t world, uint32_t tiles_x, uint32_t xbound, uint32_t height, uint32_t width,
                           uint32_t total, uint32_t stride_px, uint32_t n_tiles);
hipError_t launch_variance(hipStream_t st, const float4* accum, const float2* tile_plan, float* out, uint32_t n_slots,
                           uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound, uint32_t height,
                           const unsigned long long* error_flag);
hipError_t launch_assemble_plane(hipStream_t st, const float* gathered, float* frame, const uint32_t* rank_base,
                                 uint32_t world, uint32_t tiles_x, uint32_t xbound, uint32_t height, uint32_t width,
                                 uint32_t total, uint32_t stride_px, uint32_t n_tiles);
hipError_t launch_features_error(hipStream_t st, float4* out, uint64_t n_f4, const unsigned long long* error_flag);
// zrt_ctx_trace's end: slot -> list index, or NaN / -1 behind a launch that set *error_flag
hipError_t launch_trace_finish(hipStream_t st, float* t, int32_t* prim, uint32_t n, const uint32_t* slot_prim,
                               const unsigned long long* error_flag);
// zrt_ctx_occluded's: 0xFF in every byte behind a launch that set *error_flag
hipError_t launch_anyhit_error(hipStream_t st, uint8_t* out, uint32_t n, const unsigned long long* error_flag);
// zrt_ctx_ao's: the count plane folded into the result, or 0xFFFFFFFF / NaN in D behind a launch that set *error_flag
hipError_t launch_ao_finish(hipStream_t st, const AoArgs& g, uint32_t width, uint32_t height, uint32_t xbound,
                            const float4* feat, uint32_t* clear, float* ao, const uint32_t* plane,
                            const unsigned long long* error_flag);
// zrt_ctx_radiance's: n_chunks parked chunk sums ([chunk][ray]) folded into sum in chunk order (from 0 where
// zero_first); final: rgb = sum * scale, or NaN in sum.rgb and rgb behind a launch that set *error_flag
hipError_t launch_radiance_finish(hipStream_t st, const float4* partial, uint32_t n, uint32_t n_chunks,
                                  uint32_t zero_first, float4* sum, float* rgb, float scale, uint32_t final,
                                  const unsigned long long* error_flag);
// zrt_ctx_camera's: launch_radiance_finish over the slots of g (n_items is not read), slot -> pixel; only the
// rectangle's pixels of sum and rgb (whole-frame buffers indexed by R) are read or written
// moments (zrt_ctx_camera_moments): sum.w carries Q over the first q_chunks of the round's parked sums
hipError_t launch_camera_finish(hipStream_t st, const float4* partial, const CameraArgs& g, uint32_t n_chunks,
                                uint32_t zero_first, float4* sum, float* rgb, float scale, uint32_t final,
                                const unsigned long long* error_flag, uint32_t moments, uint32_t q_chunks);
// lens_features_kernel<mode, stack width> (zrt_ctx_camera_features): anyhit_kernel's modes; g: the rectangle, its
// slots (n, tiles_w) and the lens (the sample fields are not read)
void* lens_features_kernel_ptr(int mode, bool stk16);
// zrt_ctx_camera_features': NaN in the rectangle's floats behind a launch that set *error_flag
hipError_t launch_lens_features_error(hipStream_t st, float4* out, const CameraArgs& g,
                                      const unsigned long long* error_flag);
hipError_t launch_debug_math(int fn, const float* x, const float* y, float* out, uint32_t n);
hipError_t launch_debug_division(uint64_t n, unsigned long long* counts);
hipError_t launch_debug_rng(uint32_t prng, uint64_t key, unsigned long long* out, uint32_t n);
// schedule_tiles' stable descending radix sort of (cost, tile id) pairs (hipcub); temp == nullptr: its size only
hipError_t sort_tiles(void* temp, size_t* temp_bytes, const uint32_t* cost, uint32_t* cost_sorted, const uint32_t* ids,
                      uint32_t* order, uint32_t n, hipStream_t st);
}  // namespace zrt
