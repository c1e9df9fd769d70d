// Host ASan + UBSan harness ("Race detection / sanitizers":
// host ASan/UBSan builds of the CPU restatement).  The reference relies on Zig's
// ReleaseSafe checks (build.zig:12); the host half of this repository is C/C++, so
// its equivalent is a sanitizer build of every host source that touches scene
// data, driven through the same C ABI the GPU path uses:
//
//   scene_io.cpp   zrt_scene_load (scenes.zig / obj_reader.zig), zrt_scene_write/read
//   image_io.cpp   zrt_image_read_png / write_png / write_ppm (png_image.zig)
//   bvh_build.cpp  zrt_bvh_build (bvh.zig:62-185)
//   accel_build.cpp  the wide tree over the reference leaves (render.hip's FAST layout)
//   planner.cpp, flatten.cpp, debug_plans.cpp  the LDS / buffer / launch / pass /
//                  adaptive planners and the scene flattener, through the zrt_debug_*
//                  entry points that need no device; the per-tile walk directly
//   radiance.cpp   its part that needs no device (-DZRT_PLAN_ONLY): plan_radiance through
//                  zrt_debug_radiance_plan, zrt_rays_equirect
//   camera_query.cpp its part that needs no device: plan_camera through zrt_debug_camera_plan,
//                  zrt_lens_check, zrt_lens_init, zrt_lens_from_camera
//   oracle/        oracle_render (both RNG modes), oracle_render_scanlines,
//                  oracle_trace, oracle_bvh_build
//
// and, after the reference scenes, the degenerate families of tests/degenerate_scenes.py
// (flat leaves, duplicates, zero-size and non-finite boxes) through the same calls.
//
// Device code is not built here (GPU sanitizers are not available on the pool);
// build_bvh_device is stubbed to "not available", which is what the host build
// path does without a GPU, and kernel_config() (render.hip's) returns the values the
// shipped kernels are built with.  Any sanitizer report aborts with a non-zero status
// (-fno-sanitize-recover=all); tests/test_sanitizers.py builds and runs this.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/zrt.h"
#include "../../oracle/oracle.h"
#include "../../zraytrace_amd/csrc/accel_build.hpp"
#include "../../zraytrace_amd/csrc/bvh_build.hpp"
#include "../../zraytrace_amd/csrc/host.hpp"
#include "../../zraytrace_amd/csrc/kernels.hpp"

namespace zrt {
bool build_bvh_device(const zrt_prim*, uint32_t, int, BuiltBvh*) { return false; }
// render.hip's defaults: its #ifndef values, and the sizes that follow from them
const KernelConfig& kernel_config() {
  static const KernelConfig k = [] {
    KernelConfig c{};
    c.waves_wide = 6, c.waves_wf = 4, c.waves_pool = 4, c.waves_list = 6, c.waves_per_simd = 8;
    c.att_rows_lock = 4, c.att_rows_wf = 12, c.att_rows_pool = 3, c.att_rows_list = 24;
    c.stack_rows_lock = 16, c.sync_samples = 1, c.probe_spp = 1;
    c.oct_copies = 8;
    c.lane_words[0] = 4 + 5, c.lane_words[1] = 8 + 5;  // Rng<PRNG>'s words + 5 (LaneState)
    c.block_paths = 128 * 4;                           // kPoolPaths per wave x 4 waves
    c.layout = kLayoutVersion | kLayoutSphereSlots | kLayoutSphereFirst;
    c.paxis_m = 1024.0f;
    return c;
  }();
  return k;
}
}  // namespace zrt
// the C++ scene API's render() (zrt.hpp) forwards here; nothing in this harness calls it
extern "C" int zrt_render(const zrt_scene*, const zrt_camera*, const zrt_params*, float*, zrt_stats*) {
  return ZRT_E_NODEVICE;
}

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      std::fprintf(stderr, __VA_ARGS__);         \
      std::fprintf(stderr, "\n");                \
      ++g_fail;                                  \
    }                                            \
  } while (0)

static zrt_params params(uint32_t w, uint32_t h, uint32_t spp, uint32_t depth, uint32_t rng) {
  zrt_params p;
  std::memset(&p, 0, sizeof p);
  p.width = w;
  p.height = h;
  p.samples_per_pixel = spp;
  p.max_depth = depth;
  p.bounded_volume_hierarchy = 1;
  p.rng_mode = rng;
  p.seed = 42;
  p.world_size = 1;
  p.sample_chunk = 3;
  return p;
}

// the reference BVH's leaves in DFS order, as flatten.cpp's flatten_scene hands
// them to build_wide_bvh (refs are placeholders: the builder only carries them)
static uint32_t wide_tree(const zrt::BuiltBvh& bvh) {
  std::vector<zrt::RefLeaf> leaves;
  for (const zrt::BuildNode& b : bvh.nodes) {
    if (b.left >= 0) continue;
    zrt::RefLeaf L;
    for (int k = 0; k < 3; ++k) {
      L.mn[k] = b.mn[k];
      L.mx[k] = b.mx[k];
    }
    L.prim_a = b.left;
    L.prim_b = b.right;
    leaves.push_back(L);
  }
  const zrt::WideBvh w = zrt::build_wide_bvh(leaves);
  return w.n_nodes;
}

static void one_scene(uint32_t index, const std::string& assets, const std::string& tmp) {
  zrt_scene_data* data = nullptr;
  zrt_camera cam;
  int rc = zrt_scene_load(index, assets.c_str(), &data, &cam);
  CHECK(rc == ZRT_OK, "scene %u: %s", index, zrt_last_error());
  if (rc) return;
  const zrt_scene* s = zrt_scene_view(data);

  // host BVH build (bvh.zig:62-185) == the oracle's comparison-sort build
  zrt_bvh_node* nodes = nullptr;
  uint32_t n_nodes = 0, depth = 0;
  rc = zrt_bvh_build(s, &nodes, &n_nodes, &depth);
  CHECK(rc == ZRT_OK, "scene %u bvh: %s", index, zrt_last_error());
  zrt_bvh_node* onodes = nullptr;
  uint32_t on = 0, od = 0;
  if (s->n_prims > 10) {
    rc = oracle_bvh_build(s, &onodes, &on, &od);
    CHECK(rc == 0 && on == n_nodes && od == depth && std::memcmp(nodes, onodes, sizeof(zrt_bvh_node) * on) == 0,
          "scene %u: host BVH differs from the oracle's", index);
    const zrt::BuiltBvh built = zrt::build_bvh(s->prims, s->n_prims);
    CHECK(built.nodes.size() == n_nodes, "scene %u: build_bvh node count", index);
    CHECK(wide_tree(built) > 0, "scene %u: empty wide tree", index);
  }
  zrt_free(nodes);
  oracle_free(onodes);

  // oracle renders: counter mode (the GPU's partner) and the reference stream
  for (uint32_t rng : {uint32_t(ZRT_RNG_COUNTER), uint32_t(ZRT_RNG_REFERENCE_STREAM)}) {
    const zrt_params p = params(12, 9, 3, 6, rng);
    std::vector<float> img(size_t(p.width) * p.height * 3);
    zrt_stats st;
    rc = oracle_render(s, &cam, &p, img.data(), &st);
    CHECK(rc == 0 && st.pixels_processed > 0 && st.samples_processed == st.pixels_processed * p.samples_per_pixel,
          "scene %u rng %u: oracle_render rc %d", index, rng, rc);
    std::vector<zrt_scanline> rows(p.height);
    rc = oracle_render_scanlines(s, &cam, &p, img.data(), &st, rows.data());
    CHECK(rc == 0, "scene %u rng %u: oracle_render_scanlines rc %d", index, rng, rc);
  }

  // closest-hit queries through both of the oracle's surface structures
  std::vector<float> rays;
  for (int i = 0; i < 64; ++i) {
    const float a = 0.1f * float(i);
    const float r[6] = {cam.origin.x, cam.origin.y, cam.origin.z, std::sin(a) * 0.3f, std::cos(a) * 0.2f - 0.1f, -1.f};
    rays.insert(rays.end(), r, r + 6);
  }
  std::vector<float> t(64);
  std::vector<int32_t> surf(64);
  for (int bvh = 0; bvh < 2; ++bvh) {
    rc = oracle_trace(s, bvh, rays.data(), 64, t.data(), surf.data());
    CHECK(rc == 0, "scene %u: oracle_trace(bvh=%d) rc %d", index, bvh, rc);
  }

  // the planners and the flattener (planner.cpp, flatten.cpp) through the no-device
  // debug entry points: every LDS plan, both buffer sizings, the launch decision
  uint32_t n_plans = 0;
  rc = zrt_debug_lds_plans(s, &n_plans);
  CHECK(rc == ZRT_OK && n_plans > 0, "scene %u lds plans: %s", index, zrt_last_error());
  for (uint32_t legacy : {0u, 1u}) {
    rc = zrt_debug_buffer_plans(s, legacy, &n_plans);
    // (legacy = 1 is the sizing the check exists to refuse: either answer, no report)
    CHECK(legacy ? (rc == ZRT_OK || rc == ZRT_E_UNSUPPORTED) : rc == ZRT_OK, "scene %u buffer plans (legacy %u): %s",
          index, legacy, zrt_last_error());
  }
  for (uint32_t trav : {uint32_t(ZRT_TRAVERSAL_FAST), uint32_t(ZRT_TRAVERSAL_BINARY), uint32_t(ZRT_TRAVERSAL_REFERENCE)})
    for (uint32_t depth : {0u, 1u, 30u})
      for (uint32_t prng : {uint32_t(ZRT_PRNG_XOROSHIRO128), uint32_t(ZRT_PRNG_XOSHIRO256)}) {
        zrt_params p = params(64, 48, 256, depth, ZRT_RNG_COUNTER);
        p.traversal = trav;
        p.prng = prng;
        zrt_launch_plan lp;
        rc = zrt_debug_launch_plan(s, &p, &lp);
        CHECK(rc == ZRT_OK && lp.lds_bytes <= (160u << 10), "scene %u launch plan (traversal %u depth %u prng %u): %s",
              index, trav, depth, prng, zrt_last_error());
        uint32_t lean = 0;
        rc = zrt_debug_lean_kernel(s, &cam, &p, &lean);
        CHECK(rc == ZRT_OK, "scene %u lean kernel: %s", index, zrt_last_error());
        // the tile classifier (tile_class.cpp), ragged tiles, one rank and the second of three
        for (uint32_t world : {1u, 3u}) {
          zrt_params q = p;
          q.world_size = world;
          q.rank = world - 1;
          std::vector<uint32_t> cls(64);
          uint32_t n_tiles = 0, n_sky = 0;
          double margins[4];
          rc = zrt_debug_tile_classes(s, &cam, &q, cls.data(), uint32_t(cls.size()), &n_tiles, &n_sky, margins);
          CHECK(rc == ZRT_OK && n_sky <= n_tiles, "scene %u tile classes: %s", index, zrt_last_error());
          // the one-sphere class: one sphere per call, never on a sky tile, none where the launch is not eligible
          uint32_t n_one = 0, word = 0;
          for (uint32_t i = 0; i < n_tiles && i < cls.size(); ++i) {
            if (cls[i] == ZRT_TILE_SKY || !(cls[i] & ZRT_TILE_ONE_SPHERE)) continue;
            CHECK(!(cls[i] & ZRT_TILE_SKY) && (n_one == 0 || cls[i] == word), "scene %u: class word %08x beside %08x",
                  index, cls[i], word);
            word = cls[i];
            ++n_one;
          }
          CHECK(n_one + n_sky <= n_tiles && (n_one == 0 || (lean && depth >= 1 && trav == ZRT_TRAVERSAL_FAST)),
                "scene %u: %u one-sphere tiles (lean %u depth %u traversal %u)", index, n_one, lean, depth, trav);
        }
      }
  {  // ... and a frame large enough for its threads (1024 x 1024: 16 squares of 32 x 32 tiles)
    zrt_params q = params(1024, 1024, 4, 20, ZRT_RNG_COUNTER);
    uint32_t n_tiles = 0, n_sky = 0;
    rc = zrt_debug_tile_classes(s, &cam, &q, nullptr, 0, &n_tiles, &n_sky, nullptr);
    CHECK(rc == ZRT_OK && n_tiles == 16384 && n_sky <= n_tiles, "scene %u tile classes at 1024 x 1024: %s", index,
          zrt_last_error());
    // ... its one-sphere tiles (the threads' counts merged, one sphere kept), and the class switched off
    std::vector<uint32_t> big(n_tiles), off(n_tiles);
    uint32_t n_sky_off = 0;
    rc = zrt_debug_tile_classes(s, &cam, &q, big.data(), n_tiles, &n_tiles, &n_sky, nullptr);
    setenv("ZRT_SPHERE_TILES", "0", 1);
    const int rc_off = zrt_debug_tile_classes(s, &cam, &q, off.data(), n_tiles, &n_tiles, &n_sky_off, nullptr);
    unsetenv("ZRT_SPHERE_TILES");
    CHECK(rc == ZRT_OK && rc_off == ZRT_OK && n_sky == n_sky_off, "scene %u: sky tiles %u / %u with the one-sphere class on / off",
          index, n_sky, n_sky_off);
    uint32_t n_one = 0;
    for (uint32_t i = 0; i < n_tiles; ++i) {
      const bool one = big[i] != ZRT_TILE_SKY && (big[i] & ZRT_TILE_ONE_SPHERE);
      n_one += one;
      CHECK(off[i] == (one ? 0u : big[i]), "scene %u tile %u: class %08x, %08x with ZRT_SPHERE_TILES=0", index, i, big[i],
            off[i]);
    }
    if (index == 2) CHECK(n_one > n_tiles / 4, "scene 2: %u one-sphere tiles of %u", n_one, n_tiles);
    // the slot a class word names is a sphere's (zrt_debug_slot_prims)
    uint32_t n_slots = 0;
    rc = zrt_debug_slot_prims(s, &q, nullptr, 0, &n_slots);
    std::vector<uint32_t> slot_prim(n_slots);
    if (!rc) rc = zrt_debug_slot_prims(s, &q, slot_prim.data(), n_slots, &n_slots);
    CHECK(rc == ZRT_OK && n_slots == s->n_prims, "scene %u slot prims: %s", index, zrt_last_error());
    for (uint32_t i = 0; i < n_tiles && !rc; ++i)
      if (big[i] != ZRT_TILE_SKY && (big[i] & ZRT_TILE_ONE_SPHERE)) {
        const uint32_t slot = big[i] & (ZRT_TILE_ONE_SPHERE - 1u);
        CHECK(slot < n_slots && s->prims[slot_prim[slot]].kind == ZRT_PRIM_SPHERE, "scene %u tile %u: slot %u is no sphere",
              index, i, slot);
        break;
      }
  }
  if (s->n_prims > 10) {
    uint64_t n_slots = 0;
    rc = zrt_debug_qnodes(s, &n_slots);
    CHECK(rc == ZRT_OK && n_slots > 0, "scene %u qnodes: %s", index, zrt_last_error());
  }

  // binary scene file round trip
  const std::string path = tmp + "/scene" + std::to_string(index) + ".zrts";
  rc = zrt_scene_write(s, &cam, path.c_str());
  CHECK(rc == ZRT_OK, "scene %u write: %s", index, zrt_last_error());
  zrt_scene_data* back = nullptr;
  zrt_camera cam2;
  rc = zrt_scene_read(path.c_str(), &back, &cam2);
  CHECK(rc == ZRT_OK, "scene %u read: %s", index, zrt_last_error());
  if (!rc) {
    const zrt_scene* b = zrt_scene_view(back);
    CHECK(b->n_prims == s->n_prims && std::memcmp(b->prims, s->prims, sizeof(zrt_prim) * s->n_prims) == 0,
          "scene %u: prims differ after the round trip", index);
    CHECK(std::memcmp(&cam, &cam2, sizeof cam) == 0, "scene %u: camera differs after the round trip", index);
    zrt_scene_free(back);
  }
  zrt_scene_free(data);
}

// plan_pass / plan_adapt at the edge values of tests/test_accum_plan.py and
// tests/test_adapt_plan.py: whole and ragged passes, every refusal, chunk 0, the
// last sample of a u16 cap; the level lists, their refusals and a short array
static void pass_and_adapt_plans() {
  struct Case { uint32_t cap, chunk, w, h, done, n; bool ok; };
  const Case cases[] = {{12, 3, 24, 24, 0, 3, true},    {12, 3, 24, 24, 3, 6, true},   {12, 3, 24, 24, 9, 3, true},
                        {12, 3, 24, 24, 12, 1, false},  {10, 3, 24, 24, 6, 4, true},   {10, 3, 24, 24, 10, 1, false},
                        {12, 3, 24, 24, 10, 2, false},  {12, 3, 24, 24, 0, 0, false},  {12, 3, 24, 24, 9, 4, false},
                        {12, 3, 24, 24, 0, 13, false},  {12, 3, 24, 24, 4, 3, false},  {65536, 3, 24, 24, 0, 3, false},
                        {256, 0, 24, 24, 64, 100, true}, {256, 0, 24, 24, 16, 32, false}, {12, 3, 20, 13, 6, 4, true},
                        {12, 3, 13, 20, 0, 6, false},   {65535, 4096, 2, 2, 0, 61440, true},
                        {65535, 4096, 2, 2, 61440, 4095, true}, {65535, 4096, 2, 2, 65535, 1, false}};
  for (const Case& c : cases) {
    zrt_params p = params(c.w, c.h, c.cap, 4, ZRT_RNG_COUNTER);
    p.sample_chunk = c.chunk;
    zrt_pass_plan plan;
    const int rc = zrt_debug_pass_plan(&p, c.done, c.n, &plan);
    CHECK(c.ok ? rc == ZRT_OK && plan.samples_after == c.done + c.n : rc == ZRT_E_INVALID,
          "pass plan cap %u chunk %u done %u n %u: rc %d", c.cap, c.chunk, c.done, c.n, rc);
  }
  zrt_params p3 = params(24, 24, 12, 4, ZRT_RNG_COUNTER);
  p3.world_size = 3;
  p3.rank = 1;
  zrt_pass_plan plan;
  CHECK(zrt_debug_pass_plan(&p3, 0, 12, &plan) == ZRT_OK && plan.pass_chunks == 4, "pass plan of rank 1 of 3");
  CHECK(zrt_debug_pass_plan(nullptr, 0, 1, &plan) == ZRT_E_INVALID && zrt_debug_pass_plan(&p3, 0, 1, nullptr) == ZRT_E_INVALID,
        "pass plan: null arguments accepted");

  struct Adapt { uint32_t cap, chunk, first; float tol; uint32_t n_levels; };  // n_levels 0: refused
  const Adapt adapts[] = {{12, 3, 3, 0.5f, 3},  {48, 3, 3, 0.5f, 5},    {1024, 0, 32, 0.0f, 6}, {20, 3, 3, 0.5f, 4},
                          {48, 3, 4, 0.5f, 4},  {48, 3, 0, 0.5f, 5},    {64, 0, 1, 0.5f, 2},    {12, 3, 12, 0.5f, 1},
                          {12, 3, 4000000000u, 0.5f, 1}, {2, 3, 0, 0.5f, 1}, {12, 3, 3, 1e30f, 3},
                          {12, 3, 3, -1.0f, 0}, {12, 3, 3, NAN, 0},     {12, 3, 3, INFINITY, 0}, {65536, 3, 3, 0.5f, 0}};
  for (const Adapt& a : adapts) {
    zrt_params p = params(24, 24, a.cap, 4, ZRT_RNG_COUNTER);
    p.sample_chunk = a.chunk;
    const zrt_adaptive ad = {a.tol, a.first};
    uint32_t levels[2], n = 0;  // (a short array: the count is still the plan's)
    const int rc = zrt_debug_adapt_plan(&p, &ad, levels, 2, &n);
    CHECK(a.n_levels ? rc == ZRT_OK && n == a.n_levels : rc == ZRT_E_INVALID,
          "adapt plan cap %u chunk %u first %u: rc %d, %u levels", a.cap, a.chunk, a.first, rc, n);
  }
  const zrt_adaptive ad = {0.5f, 3};
  uint32_t n = 0;
  CHECK(zrt_debug_adapt_plan(&p3, &ad, nullptr, 0, &n) == ZRT_OK && n == 3, "adapt plan: count alone");
  CHECK(zrt_debug_adapt_plan(nullptr, &ad, nullptr, 0, &n) == ZRT_E_INVALID &&
            zrt_debug_adapt_plan(&p3, nullptr, nullptr, 0, &n) == ZRT_E_INVALID &&
            zrt_debug_adapt_plan(&p3, &ad, nullptr, 8, &n) == ZRT_E_INVALID &&
            zrt_debug_adapt_plan(&p3, &ad, nullptr, 0, nullptr) == ZRT_E_INVALID,
        "adapt plan: null arguments accepted");
}

// plan_radiance at the edge values of tests/test_radiance_plan.py: chunking, items past 32
// bits, rounds under a cap, the grid bound, every refusal; the equirectangular generator
// writing exactly width * height * 6 floats (the buffer is that long: a write past it aborts)
static void radiance_plans() {
  struct Case { uint32_t n, samples, first_sample; uint64_t first_ray; uint32_t flags, chunk, cu; uint64_t cap; bool ok; };
  const Case cases[] = {{100, 9, 0, 0, 0, 4, 256, 0, true},
                        {0xffffffffu, 4096, 0, 0, 0, 2, 256, 0, true},
                        {257, 9, 0, 0, 0, 4, 1, 257 * 16, true},
                        {1u << 20, 64, 0, 0, 0, 4, 256, 1, true},
                        {0, 5, 0, 0, 0, 2, 256, 0, true},
                        {4, 1, 65535, 0, 0, 0, 256, 0, true},
                        {3, 1, 0, (1ull << 48) - 3, 0, 0, 256, 0, true},
                        {4, 4, 8, 0, ZRT_RQ_ACCUMULATE, 4, 256, 0, true},
                        {4, 0, 0, 0, 0, 4, 256, 0, false},
                        {4, 2, 65535, 0, 0, 4, 256, 0, false},
                        {4, 1, 0, (1ull << 48) - 3, 0, 4, 256, 0, false},
                        {4, 1, 0, ~0ull, 0, 4, 256, 0, false},
                        {4, 1, 0, 0, 2, 4, 256, 0, false},
                        {4, 4, 6, 0, ZRT_RQ_ACCUMULATE, 4, 256, 0, false},
                        {4, 1, 0, 0, 0, 4, 0, 0, false}};
  for (const Case& c : cases) {
    zrt_params p = params(1, 1, 1, 8, ZRT_RNG_COUNTER);
    p.sample_chunk = c.chunk;
    struct zrt_radiance rq;
    std::memset(&rq, 0, sizeof(rq));
    rq.n_samples = c.samples;
    rq.first_sample = c.first_sample;
    rq.first_ray = c.first_ray;
    rq.flags = c.flags;
    zrt_radiance_plan plan;
    const int rc = zrt_debug_radiance_plan(&p, &rq, c.n, c.cu, c.cap, &plan);
    const bool fine = c.ok ? rc == ZRT_OK && plan.items == uint64_t(c.n) * plan.call_chunks &&
                                 (c.n == 0 || (plan.grid >= 1 && plan.grid <= plan.blocks_per_cu * c.cu &&
                                               uint64_t(plan.rounds) * plan.chunks_per_round >= plan.call_chunks &&
                                               plan.partial_bytes == uint64_t(c.n) * plan.chunks_per_round * 16))
                           : rc == ZRT_E_INVALID;
    CHECK(fine, "radiance plan n %u samples %u first %u flags %u: rc %d", c.n, c.samples, c.first_sample, c.flags, rc);
  }
  zrt_params p = params(1, 1, 1, 8, ZRT_RNG_COUNTER);
  struct zrt_radiance rq;
  std::memset(&rq, 0, sizeof(rq));
  rq.n_samples = 1;
  zrt_radiance_plan plan;
  CHECK(zrt_debug_radiance_plan(nullptr, &rq, 1, 1, 0, &plan) == ZRT_E_INVALID &&
            zrt_debug_radiance_plan(&p, nullptr, 1, 1, 0, &plan) == ZRT_E_INVALID &&
            zrt_debug_radiance_plan(&p, &rq, 1, 1, 0, nullptr) == ZRT_E_INVALID,
        "radiance plan: null arguments accepted");
  const float origin[3] = {1.5f, -2.0f, 0.25f};
  for (uint32_t w : {1u, 4u, 7u}) {
    const uint32_t h = w == 4 ? 2 : 3;
    std::vector<float> rays(size_t(w) * h * 6);
    CHECK(zrt_rays_equirect(origin, w, h, rays.data()) == ZRT_OK, "equirect %ux%u: %s", w, h, zrt_last_error());
    bool unit = true;
    for (size_t i = 0; i < size_t(w) * h; ++i) {
      const float* r = &rays[6 * i];
      const double l = double(r[3]) * r[3] + double(r[4]) * r[4] + double(r[5]) * r[5];
      unit = unit && std::fabs(l - 1.0) < 1e-6 && r[0] == origin[0] && r[1] == origin[1] && r[2] == origin[2];
    }
    CHECK(unit, "equirect %ux%u: a direction is not a unit vector or an origin moved", w, h);
  }
  CHECK(zrt_rays_equirect(origin, 0, 2, nullptr) == ZRT_E_INVALID && zrt_rays_equirect(nullptr, 1, 1, nullptr) == ZRT_E_INVALID,
        "equirect: bad arguments accepted");
}

// plan_camera at the edge values of tests/test_camera_plan.py: rectangles that are and are not
// multiples of 8, the largest frame, every refusal of the query; zrt_lens_init, zrt_lens_check
// and zrt_lens_from_camera over every kind, degenerate poses and non-finite floats
static void camera_plans() {
  struct Case { uint32_t width, height, x0, y0, w, h, samples, first_sample, flags, chunk, cu; uint64_t cap; bool ok; };
  const Case cases[] = {{24, 16, 0, 0, 24, 16, 9, 0, 0, 4, 256, 0, true},
                        {24, 16, 3, 5, 13, 9, 9, 0, 0, 4, 256, 0, true},
                        {24, 16, 23, 15, 1, 1, 1, 65535, 0, 0, 1, 0, true},
                        {40, 24, 0, 0, 40, 24, 9, 0, 0, 4, 256, 960 * 16, true},
                        {65535, 65535, 0, 0, 65535, 65527, 64, 0, 0, 4, 4, 1, true},
                        {24, 16, 0, 0, 24, 16, 8, 8, ZRT_CQ_ACCUMULATE, 4, 256, 0, true},
                        {65535, 65535, 0, 0, 65535, 65535, 1, 0, 0, 4, 256, 0, false},
                        {24, 16, 0, 0, 0, 16, 1, 0, 0, 4, 256, 0, false},
                        {24, 16, 1, 0, 24, 16, 1, 0, 0, 4, 256, 0, false},
                        {24, 16, 0xffffffffu, 0, 2, 1, 1, 0, 0, 4, 256, 0, false},
                        {24, 16, 0, 16, 1, 1, 1, 0, 0, 4, 256, 0, false},
                        {24, 16, 0, 0, 24, 16, 0, 0, 0, 4, 256, 0, false},
                        {24, 16, 0, 0, 24, 16, 2, 65535, 0, 4, 256, 0, false},
                        {24, 16, 0, 0, 24, 16, 1, 0, 2, 4, 256, 0, false},
                        {24, 16, 0, 0, 24, 16, 4, 6, ZRT_CQ_ACCUMULATE, 4, 256, 0, false},
                        {24, 16, 0, 0, 24, 16, 1, 0, 0, 4, 0, 0, false},
                        {0, 16, 0, 0, 1, 1, 1, 0, 0, 4, 256, 0, false},
                        {65536, 1, 0, 0, 1, 1, 1, 0, 0, 4, 256, 0, false}};
  for (const Case& c : cases) {
    zrt_params p = params(c.width, c.height, 1, 8, ZRT_RNG_COUNTER);
    p.sample_chunk = c.chunk;
    zrt_camera_query q;
    std::memset(&q, 0, sizeof(q));
    q.x0 = c.x0; q.y0 = c.y0; q.w = c.w; q.h = c.h;
    q.n_samples = c.samples;
    q.first_sample = c.first_sample;
    q.flags = c.flags;
    zrt_camera_plan plan;
    const int rc = zrt_debug_camera_plan(&p, &q, c.cu, c.cap, &plan);
    const bool fine = c.ok ? rc == ZRT_OK && plan.slots == uint64_t(plan.tiles_w) * plan.tiles_h * 64 && plan.slots < (1ull << 32) &&
                                 plan.pixels == uint64_t(c.w) * c.h && plan.slots >= plan.pixels &&
                                 plan.radiance.items == plan.slots * plan.radiance.call_chunks &&
                                 plan.radiance.grid >= 1 && plan.radiance.grid <= plan.radiance.blocks_per_cu * c.cu
                           : rc == ZRT_E_INVALID;
    CHECK(fine, "camera plan %ux%u rect %u %u %u %u samples %u: rc %d", c.width, c.height, c.x0, c.y0, c.w, c.h, c.samples, rc);
  }
  zrt_params p = params(8, 8, 1, 8, ZRT_RNG_COUNTER);
  zrt_camera_query q;
  std::memset(&q, 0, sizeof(q));
  q.w = q.h = q.n_samples = 1;
  zrt_camera_plan plan;
  CHECK(zrt_debug_camera_plan(nullptr, &q, 1, 0, &plan) == ZRT_E_INVALID && zrt_debug_camera_plan(&p, nullptr, 1, 0, &plan) == ZRT_E_INVALID &&
            zrt_debug_camera_plan(&p, &q, 1, 0, nullptr) == ZRT_E_INVALID,
        "camera plan: null arguments accepted");
  const float from[3] = {0.4f, 1.7f, -3.6f}, at[3] = {0.1f, 0.2f, 0.0f}, up[3] = {0.0f, 1.0f, 0.0f};
  zrt_camera cam;
  CHECK(zrt_camera_init(from, at, up, 40.0f, 1.5f, &cam) == ZRT_OK, "camera_init: %s", zrt_last_error());
  for (uint32_t kind = 0; kind <= ZRT_LENS_FISHEYE; ++kind) {
    zrt_lens l, m;
    CHECK(zrt_lens_init(kind, from, at, up, 40.0f, 1.5f, 0.3f, 1.0f, 180.0f, &l) == ZRT_OK && zrt_lens_check(&l) == ZRT_OK,
          "lens_init kind %u: %s", kind, zrt_last_error());
    CHECK(std::memcmp(&l.lower_left_corner, &cam.lower_left_corner, sizeof(zrt_vec3) * 3) == 0 &&
              std::memcmp(&l.origin, &cam.origin, sizeof(zrt_vec3)) == 0,
          "lens_init kind %u: the plane at focus_dist 1 is not zrt_camera_init's", kind);
    CHECK(zrt_lens_from_camera(kind, &cam, 0.3f, 0.0f, 180.0f, &m) == ZRT_OK &&
              std::memcmp(&m.lower_left_corner, &cam.lower_left_corner, sizeof(zrt_vec3) * 3) == 0,
          "lens_from_camera kind %u: %s", kind, zrt_last_error());
    CHECK(zrt_lens_from_camera(kind, &cam, 0.3f, 2.5f, 120.0f, &m) == ZRT_OK && zrt_lens_check(&m) == ZRT_OK,
          "lens_from_camera kind %u at a focal distance: %s", kind, zrt_last_error());
    CHECK(zrt_lens_init(kind, from, from, up, 40.0f, 1.5f, 0.0f, 1.0f, 180.0f, &l) == ZRT_E_INVALID &&
              zrt_lens_init(kind, from, at, up, 40.0f, 1.5f, 0.0f, 1.0f, 0.0f, &l) == ZRT_E_INVALID &&
              (kind == ZRT_LENS_ORTHO || kind == ZRT_LENS_FISHEYE ||  // (their axes are the frame's: no aperture)
               zrt_lens_init(kind, from, at, up, 40.0f, 1.5f, INFINITY, 1.0f, 180.0f, &l) == ZRT_E_INVALID) &&
              zrt_lens_init(kind, from, at, up, 40.0f, 1.5f, 0.0f, NAN, 180.0f, &l) == ZRT_E_INVALID &&
              zrt_lens_init(kind, nullptr, at, up, 40.0f, 1.5f, 0.0f, 1.0f, 180.0f, &l) == ZRT_E_INVALID,
          "lens_init kind %u: a degenerate pose, field of view or aperture accepted", kind);
    zrt_camera flat = cam;
    flat.horizontal = zrt_vec3{0.0f, 0.0f, 0.0f};
    CHECK(zrt_lens_from_camera(kind, &flat, 0.0f, 0.0f, 180.0f, &m) == ZRT_E_INVALID, "lens_from_camera kind %u: a flat plane accepted", kind);
  }
  zrt_lens l;
  CHECK(zrt_lens_init(5, from, at, up, 40.0f, 1.5f, 0.0f, 1.0f, 180.0f, &l) == ZRT_E_INVALID && zrt_lens_check(nullptr) == ZRT_E_INVALID &&
            zrt_lens_from_camera(5, &cam, 0.0f, 0.0f, 180.0f, &l) == ZRT_E_INVALID,
        "lens: an unknown kind or a null lens accepted");
  // zrt_rect_check (planner.cpp): rectangles at the frame's edges, the largest frame, a frame
  // taller than wide, every refusal
  zrt_params rp = p;
  rp.width = 33;
  rp.height = 40;
  const zrt_rect in[] = {{0, 0, 33, 40}, {32, 39, 1, 1}, {5, 3, 28, 37}}, out[] = {{0, 0, 0, 1}, {0, 0, 1, 0}, {33, 0, 1, 1},
                        {0, 40, 1, 1}, {5, 3, 29, 1}, {5, 3, 1, 38}, {0xFFFFFFFFu, 0, 2, 1}, {1, 1, 0xFFFFFFFFu, 0xFFFFFFFFu}};
  for (const zrt_rect& r : in) CHECK(zrt_rect_check(&rp, &r) == ZRT_OK, "rect_check: %s", zrt_last_error());
  for (const zrt_rect& r : out) CHECK(zrt_rect_check(&rp, &r) == ZRT_E_INVALID, "rect_check: {%u, %u, %u, %u} accepted", r.x0, r.y0, r.w, r.h);
  rp.width = rp.height = 65535;
  const zrt_rect last{65534, 65534, 1, 1};
  CHECK(zrt_rect_check(&rp, &last) == ZRT_OK, "rect_check at 65535: %s", zrt_last_error());
  rp.height = 65536;
  CHECK(zrt_rect_check(&rp, &last) == ZRT_E_INVALID && zrt_rect_check(nullptr, &last) == ZRT_E_INVALID &&
            zrt_rect_check(&p, nullptr) == ZRT_E_INVALID,
        "rect_check: a 65536-row frame or a null argument accepted");
}

// plan_reproject at the cases of tests/test_temporal_host.py: a scene's camera, the
// same mirrored (s changes sign, the plan stays valid), parallel axes, a NaN, nulls
static void reproject_plans(const std::string& assets) {
  zrt_scene_data* d = nullptr;
  zrt_camera cam;
  CHECK(zrt_scene_load(1, assets.c_str(), &d, &cam) == ZRT_OK, "scene 1: %s", zrt_last_error());
  zrt_scene_free(d);
  const zrt_params p = params(24, 24, 1, 1, ZRT_RNG_COUNTER);
  zrt_reproject_plan a, b;
  CHECK(zrt_debug_reproject_plan(&cam, &p, &a) == ZRT_OK && a.valid == 1, "reproject plan: scene camera");
  zrt_camera m = cam;
  m.lower_left_corner = {cam.lower_left_corner.x + cam.horizontal.x, cam.lower_left_corner.y + cam.horizontal.y,
                         cam.lower_left_corner.z + cam.horizontal.z};
  m.horizontal = {-cam.horizontal.x, -cam.horizontal.y, -cam.horizontal.z};
  CHECK(zrt_debug_reproject_plan(&m, &p, &b) == ZRT_OK && b.valid == 1 && (a.s < 0.0f) != (b.s < 0.0f),
        "reproject plan: mirrored camera (s %g, %g)", double(a.s), double(b.s));
  m = cam;
  m.vertical = m.horizontal;
  CHECK(zrt_debug_reproject_plan(&m, &p, &b) == ZRT_OK && b.valid == 0, "reproject plan: parallel axes are valid");
  m = cam;
  m.origin.y = NAN;
  CHECK(zrt_debug_reproject_plan(&m, &p, &b) == ZRT_OK && b.valid == 0, "reproject plan: a NaN origin is valid");
  CHECK(zrt_debug_reproject_plan(nullptr, &p, &b) == ZRT_E_INVALID &&
            zrt_debug_reproject_plan(&cam, nullptr, &b) == ZRT_E_INVALID &&
            zrt_debug_reproject_plan(&cam, &p, nullptr) == ZRT_E_INVALID,
        "reproject plan: null arguments accepted");
}

// for_rank_tiles (the pixel count of a launch, zrt_ctx_scanlines) against a count over
// the frame's pixels: ragged frames, world sizes 1 - 3, every rank, a rank with no tile
static void tile_walks() {
  struct Case { uint32_t w, h, world; };
  for (const Case& k : {Case{13, 21, 1}, Case{13, 21, 2}, Case{13, 21, 3}, Case{20, 13, 3}, Case{5, 5, 3}})
    for (uint32_t rank = 0; rank < k.world; ++rank) {
      const zrt_params p = params(k.w, k.h, 1, 1, ZRT_RNG_COUNTER);
      const zrt::Geometry g = zrt::geometry(&p);
      std::vector<uint32_t> want(k.h, 0), got(k.h, 0);  // this rank's pixels in each row
      uint32_t want_tiles = 0;
      for (uint32_t y = 0; y < k.h; ++y)
        for (uint32_t x = 0; x < g.xbound; ++x) {
          const uint32_t t = (y / 8) * g.tiles_x + x / 8;
          if (t % k.world != rank) continue;
          want[y] += 1;
          want_tiles += (x % 8 == 0 && y % 8 == 0) ? 1 : 0;
        }
      uint32_t n = 0;
      bool in_order = true;
      zrt::for_rank_tiles(g, k.h, rank, k.world, [&](uint32_t lt, uint32_t w, uint32_t h, uint32_t y0) {
        in_order = in_order && lt == n && w >= 1 && w <= 8 && h >= 1 && h <= 8 && y0 + h <= k.h;
        ++n;
        for (uint32_t y = y0; y < y0 + h && y < k.h; ++y) got[y] += w;
      });
      CHECK(in_order && n == want_tiles && n == zrt::rank_tiles(g, rank, k.world) && got == want,
            "tile walk %u x %u, rank %u of %u: %u tiles (%u expected)", k.w, k.h, rank, k.world, n, want_tiles);
    }
}

// ---- degenerate geometry (tests/degenerate_scenes.py's families, built here again) ------
//
// Flat leaves, duplicates, zero-size and non-finite boxes through the host BVH build
// (against the oracle's), the wide-tree builder, the planners, the compressed-node
// encoder and the oracle's two closest-hit paths, with the oracle-side conditions of
// tests/test_degenerate_host.py.  Rays: an LCG's, aimed into the family's box.
namespace degenerate {

struct Family {
  std::string name;
  std::vector<zrt_prim> prims;
  std::vector<uint32_t> marked;  // flat / point / sliver / non-finite primitives
  float lo[3], hi[3];            // the box rays are aimed into
  int flat_axis = -1;            // flat-*: the grid's axis
  float level = 0.0f;
  bool from_above = false, from_front = false;
  uint32_t n_materials = 3;
};

static zrt_vec3 v3(double x, double y, double z) { return {float(x), float(y), float(z)}; }

static zrt_prim sphere(zrt_vec3 c, float r) {
  zrt_prim p;
  std::memset(&p, 0, sizeof p);
  p.kind = ZRT_PRIM_SPHERE;
  p.center = c;
  p.radius = r;
  return p;
}

static zrt_prim tri(zrt_vec3 a, zrt_vec3 b, zrt_vec3 c) {
  zrt_prim p;
  std::memset(&p, 0, sizeof p);
  p.kind = ZRT_PRIM_TRIANGLE;
  p.a = a, p.b = b, p.c = c;
  return p;
}

// n x n quads in the plane coordinate[axis] == level over [lo, hi]^2 (+ shift); e1 x e2 along +axis
static void quad_grid(std::vector<zrt_prim>& out, int axis, double level, int n, double lo, double hi, double su = 0.0,
                      double sv = 0.0) {
  int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
  if (axis == 1) std::swap(u, v);
  auto pt = [&](double a, double b) {
    double p[3] = {0.0, 0.0, 0.0};
    p[axis] = level, p[u] = a + su, p[v] = b + sv;
    return v3(p[0], p[1], p[2]);
  };
  std::vector<double> xs;
  for (int k = 0; k <= n; ++k) xs.push_back(lo + (hi - lo) * k / n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      out.push_back(tri(pt(xs[i], xs[j]), pt(xs[i + 1], xs[j]), pt(xs[i + 1], xs[j + 1])));
      out.push_back(tri(pt(xs[i], xs[j]), pt(xs[i + 1], xs[j + 1]), pt(xs[i], xs[j + 1])));
    }
}

static void scatter(std::vector<zrt_prim>& out, int n, double phase) {
  for (int i = 0; i < n; ++i)
    out.push_back(sphere(v3(1.2 * std::sin(1.7 * i + phase), 0.5 * std::sin(2.3 * i + 0.5 * phase), 1.2 * std::cos(1.1 * i + phase)),
                         float(0.15 + 0.025 * ((7 * i + int(phase)) % 10))));
}

static void box(Family& f, double x0, double y0, double z0, double x1, double y1, double z1) {
  f.lo[0] = float(x0), f.lo[1] = float(y0), f.lo[2] = float(z0);
  f.hi[0] = float(x1), f.hi[1] = float(y1), f.hi[2] = float(z1);
}

static Family build(const std::string& name) {
  Family f;
  f.name = name;
  box(f, -2.0, -1.0, -2.0, 2.0, 1.5, 2.0);
  std::vector<zrt_prim>& P = f.prims;
  if (name == "eleven" || name == "ten") {
    const zrt_prim s[5] = {sphere(v3(0.0, -100.5, 0.0), 100.0f), sphere(v3(-1.2, 0.0, 0.3), 0.5f),
                           sphere(v3(1.1, -0.1, -0.4), 0.4f), sphere(v3(0.0, 0.9, -1.0), 0.35f),
                           sphere(v3(0.3, -0.3, 1.0), 0.2f)};
    const zrt_prim t[6] = {tri(v3(-0.6, -0.5, -0.2), v3(0.4, -0.5, 0.6), v3(0.0, 0.5, 0.0)),
                           tri(v3(0.4, -0.5, 0.6), v3(0.7, -0.5, -0.5), v3(0.0, 0.5, 0.0)),
                           tri(v3(0.7, -0.5, -0.5), v3(-0.6, -0.5, -0.2), v3(0.0, 0.5, 0.0)),
                           tri(v3(-2.0, -0.45, 1.0), v3(-1.0, -0.45, 1.6), v3(-1.6, 0.4, 1.2)),
                           tri(v3(1.5, -0.4, 0.8), v3(2.2, -0.4, 0.2), v3(1.9, 0.6, 0.6)),
                           tri(v3(-0.5, 1.0, 0.5), v3(0.5, 1.0, 0.5), v3(0.0, 1.4, -0.2))};
    P = {s[0], t[0], s[1], t[1], t[2], s[2], t[3], s[3], t[4], s[4], t[5]};
    if (name == "ten") P.pop_back();
  } else if (name.rfind("flat-", 0) == 0) {
    f.flat_axis = name[5] - 'x';
    f.level = 0.25f;
    quad_grid(P, f.flat_axis, 0.25, 6, -1.5, 1.5);
    for (uint32_t i = 0; i < 72; ++i) f.marked.push_back(i);
    box(f, -2.0, -2.0, -2.0, 2.0, 2.0, 2.0);
  } else if (name == "terraces") {
    const double ys[3] = {-0.5, 0.0, 0.5};
    for (int k = 0; k < 3; ++k) quad_grid(P, 1, ys[k], 3, -0.9, 0.9, 0.7 * (k - 1), -0.5 * (k - 1));
    for (uint32_t i = 0; i < P.size(); ++i) f.marked.push_back(i);
    P.push_back(tri(v3(-2.0, -0.6, -1.8), v3(-2.0, -0.2, -0.6), v3(-1.0, -0.6, -1.8)));
    P.push_back(tri(v3(1.6, -0.4, 1.0), v3(1.6, 0.3, 2.0), v3(2.4, -0.4, 1.0)));
    P.push_back(tri(v3(-1.8, 0.1, 1.2), v3(-1.8, 0.6, 2.0), v3(-0.8, 0.1, 1.2)));
    P.push_back(tri(v3(0.9, 0.6, -2.0), v3(0.9, 0.9, -1.2), v3(1.9, 0.6, -2.0)));
    P.push_back(tri(v3(-0.3, -0.9, 1.6), v3(-0.3, -0.7, 2.4), v3(0.6, -0.9, 1.6)));
    P.push_back(tri(v3(-2.4, 0.7, -0.2), v3(-2.4, 0.9, 0.5), v3(-1.6, 0.7, -0.2)));
    P.push_back(sphere(v3(1.6, 0.0, -0.4), 0.45f));
    f.from_above = true;
    box(f, -2.5, -1.0, -2.5, 2.5, 1.0, 2.5);
  } else if (name == "duplicates") {
    for (int i = 0; i < 9; ++i) P.push_back(sphere(v3(-0.6, 0.0, 0.0), 0.55f));
    for (int i = 0; i < 40; ++i) P.push_back(tri(v3(0.1, -0.6, -0.3), v3(1.5, -0.6, 0.2), v3(0.7, 0.8, 0.0)));
    f.n_materials = 4;
    box(f, -1.3, -0.8, -0.6, 1.6, 0.9, 0.6);
  } else if (name == "points") {
    const zrt_vec3 pt = v3(0.25, 0.125, -0.5);
    for (int i = 0; i < 8; ++i) {
      for (int k = 0; k < 3; ++k) f.marked.push_back(uint32_t(P.size())), P.push_back(sphere(pt, 0.0f));
      f.marked.push_back(uint32_t(P.size())), P.push_back(tri(pt, pt, pt));
      if (i == 3) {
        P.push_back(sphere(v3(-0.7, 0.0, 0.0), 0.6f));
        P.push_back(tri(v3(0.0, -0.7, -0.4), v3(1.6, -0.7, 0.0), v3(0.8, 0.9, -0.2)));
      }
    }
    box(f, -1.4, -0.8, -0.7, 1.7, 1.0, 0.7);
  } else if (name == "slivers") {
    for (int k = 0; k < 12; ++k) {
      const double x0 = -1.5 + 0.25 * k, x1 = -1.0 + 0.25 * k, zc = 0.25 * (k % 3) - 0.25;
      const zrt_vec3 a = v3(x0, -0.5, zc), b = v3(x1, -0.5, zc), c = v3(x0, 0.75, zc - 0.5);
      P.push_back(tri(a, b, c));
      f.marked.push_back(uint32_t(P.size()));
      if (k % 3 == 0) P.push_back(tri(a, b, v3(0.5 * (x0 + x1), -0.5, zc)));
      else if (k % 3 == 1) P.push_back(tri(a, a, c));
      else P.push_back(tri(v3(x0, 0.0, 0.5), v3(x0 + 0.5, 0.25, 0.5), v3(x0 + 1.0, 0.5, 0.5)));
    }
    f.from_front = true;
    box(f, -1.6, -0.6, -0.9, 1.6, 0.8, 0.6);
  } else if (name == "range") {
    const double big = 8.0e18;
    P.push_back(sphere(v3(1e-30, 1e-30, 1e-30), 1e-38f));
    scatter(P, 12, 3.0);
    P.push_back(tri(v3(3.0e38, -1.0, -3.0e38), v3(2.0e38, -1.0, 3.0e38), v3(3.2e38, -1.0, 0.0)));
    P.push_back(tri(v3(-big, -0.75, -big), v3(-big, -0.75, big), v3(big, -0.75, -big)));
    f.marked = {0, 13};
    box(f, -1.5, -0.7, -1.5, 1.5, 0.8, 1.5);
  } else if (name == "inf-vertex" || name == "inf-radius") {
    scatter(P, 20, 5.0);
    const zrt_prim odd = name == "inf-vertex" ? tri(v3(0.0, -0.5, 0.0), v3(INFINITY, -0.5, 0.0), v3(0.0, 0.5, -1.0))
                                              : sphere(v3(0.0, 0.0, -3.0), INFINITY);
    P.insert(P.begin() + 10, odd);
    f.marked = {10};
    box(f, -1.6, -1.0, -1.6, 1.6, 1.0, 1.6);
  } else {  // nan-vertex, nan-center
    for (int j = 0; j < 4; ++j)
      for (int i = 0; i < 5; ++i) P.push_back(sphere(v3(-1.2 + 0.6 * i, -0.45 + 0.45 * j, -0.3 * (i % 2)), 0.2f));
    if (name == "nan-vertex") P.push_back(tri(v3(0.0, 0.0, -1.0), v3(NAN, 0.0, -1.0), v3(0.0, 1.0, -1.0)));
    else P.push_back(sphere(v3(NAN, 0.3, -0.6), 0.25f));
    f.marked = {20};
    box(f, -1.5, -0.8, -0.8, 1.5, 1.2, 0.4);
  }
  for (uint32_t i = 0; i < P.size(); ++i) P[i].material = i % f.n_materials;
  return f;
}

struct Lcg {
  uint64_t s;
  double next() {  // [0, 1)
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return double(s >> 11) * (1.0 / 9007199254740992.0);
  }
};

// 6000 rays: from a shell around the box at points inside it (flat-*: on the plane);
// every 20th ray of a flat family lies in the plane (d_k = 0, o_k on it: NaN slabs)
static std::vector<float> rays_of(const Family& f, uint32_t n) {
  Lcg g{0x9e3779b97f4a7c15ull + f.name.size() * 1000003ull + uint64_t(f.name[f.name.size() - 1])};
  double span = 0.0;
  for (int k = 0; k < 3; ++k) span = std::max(span, double(f.hi[k]) - double(f.lo[k]));
  std::vector<float> r;
  for (uint32_t i = 0; i < n; ++i) {
    double t[3], v[3], len = 0.0;
    for (int k = 0; k < 3; ++k) t[k] = f.lo[k] + (double(f.hi[k]) - f.lo[k]) * g.next();
    if (f.flat_axis >= 0) t[f.flat_axis] = f.level;
    do {
      len = 0.0;
      for (int k = 0; k < 3; ++k) v[k] = 2.0 * g.next() - 1.0, len += v[k] * v[k];
    } while (len > 1.0 || len < 1e-3);
    len = std::sqrt(len);
    for (int k = 0; k < 3; ++k) v[k] /= len;
    if (f.from_above) v[1] = std::fabs(v[1]) + 0.3;
    if (f.from_front) v[2] = std::fabs(v[2]) + 0.2;
    const bool in_plane = f.flat_axis >= 0 && i % 20 == 0;
    if (in_plane) v[f.flat_axis] = 0.0;
    const double dist = span * (0.6 + 0.8 * g.next());
    float o[3], d[3];
    for (int k = 0; k < 3; ++k) {
      o[k] = float(t[k] + v[k] * dist);
      d[k] = in_plane && k == f.flat_axis ? 0.0f : float(t[k]) - o[k];
    }
    r.insert(r.end(), o, o + 3);
    r.insert(r.end(), d, d + 3);
  }
  return r;
}

static bool is_marked(const Family& f, int32_t prim) {
  return prim >= 0 && std::find(f.marked.begin(), f.marked.end(), uint32_t(prim)) != f.marked.end();
}

static void one_family(const std::string& name) {
  const Family f = build(name);
  const char* nm = name.c_str();
  const zrt_texture texs[4] = {{ZRT_TEX_COLOR, 0, {0.8f, 0.2f, 0.15f}, 0.f, 0.f}, {ZRT_TEX_COLOR, 0, {0.8f, 0.8f, 0.85f}, 0.f, 0.f},
                               {ZRT_TEX_COLOR, 0, {0.2f, 0.7f, 0.25f}, 0.f, 0.f}, {ZRT_TEX_COLOR, 0, {0.9f, 0.9f, 0.2f}, 0.f, 0.f}};
  const zrt_material mats[4] = {{ZRT_MAT_LAMBERTIAN, 0, 0.f}, {ZRT_MAT_METAL, 1, 0.f}, {ZRT_MAT_LAMBERTIAN, 2, 0.f},
                                {ZRT_MAT_METAL, 3, 0.f}};
  zrt_scene sc;
  std::memset(&sc, 0, sizeof sc);
  sc.prims = f.prims.data();
  sc.n_prims = uint32_t(f.prims.size());
  sc.materials = mats;
  sc.n_materials = f.n_materials;
  sc.textures = texs;
  sc.n_textures = 4;
  const zrt_scene* s = &sc;
  const bool bvh = sc.n_prims > 10;
  const bool nan_mid = name == "inf-radius" || name == "nan-center";  // refused by validate_scene
  CHECK(name == "ten" ? sc.n_prims == 10 : sc.n_prims >= 11 && sc.n_prims <= 300, "%s: %u primitives", nm, sc.n_prims);

  // the host tree == the oracle's (nan-center: NaN sort keys, no tree to agree on); the wide tree
  uint32_t n_leaves = 0, n_flat = 0;
  if (bvh) {
    zrt_bvh_node *nodes = nullptr, *onodes = nullptr;
    uint32_t n_nodes = 0, depth = 0, on = 0, od = 0;
    int rc = zrt_bvh_build(s, &nodes, &n_nodes, &depth);
    CHECK(rc == ZRT_OK && n_nodes > 0, "%s bvh: %s", nm, zrt_last_error());
    rc = oracle_bvh_build(s, &onodes, &on, &od);
    CHECK(rc == 0 && on == n_nodes && od == depth, "%s: oracle tree of %u nodes, host %u", nm, on, n_nodes);
    if (name != "nan-center")
      CHECK(on == n_nodes && std::memcmp(nodes, onodes, sizeof(zrt_bvh_node) * on) == 0, "%s: host BVH differs from the oracle's", nm);
    for (uint32_t i = 0; i < on; ++i)
      if (onodes[i].left < 0) {
        ++n_leaves;
        n_flat += (onodes[i].min.x == onodes[i].max.x || onodes[i].min.y == onodes[i].max.y || onodes[i].min.z == onodes[i].max.z);
      }
    zrt_free(nodes);
    oracle_free(onodes);
    const zrt::BuiltBvh built = zrt::build_bvh(sc.prims, sc.n_prims);
    CHECK(built.nodes.size() == n_nodes && wide_tree(built) > 0, "%s: wide tree", nm);
  }

  // the planners and the encoder
  uint32_t n_plans = 0;
  uint64_t n_slots = 0;
  zrt_params p = params(24, 24, 4, 6, ZRT_RNG_COUNTER);
  zrt_launch_plan lp;
  auto refused = [&](int rc) {
    return rc == ZRT_E_UNSUPPORTED && std::strstr(zrt_last_error(), ("primitive " + std::to_string(f.marked[0]) + ":").c_str());
  };
  if (nan_mid) {
    CHECK(refused(zrt_debug_lds_plans(s, &n_plans)) && refused(zrt_debug_buffer_plans(s, 0, &n_plans)) &&
              refused(zrt_debug_launch_plan(s, &p, &lp)) && refused(zrt_debug_qnodes(s, &n_slots)),
          "%s: a NaN midpoint is not refused: %s", nm, zrt_last_error());
  } else {
    CHECK(zrt_debug_lds_plans(s, &n_plans) == ZRT_OK && n_plans > 0, "%s lds plans: %s", nm, zrt_last_error());
    CHECK(zrt_debug_buffer_plans(s, 0, &n_plans) == ZRT_OK, "%s buffer plans: %s", nm, zrt_last_error());
    for (uint32_t trav : {uint32_t(ZRT_TRAVERSAL_FAST), uint32_t(ZRT_TRAVERSAL_BINARY), uint32_t(ZRT_TRAVERSAL_REFERENCE)})
      for (uint32_t use_bvh : {1u, 0u}) {
        p.traversal = trav;
        p.bounded_volume_hierarchy = use_bvh;
        CHECK(zrt_debug_launch_plan(s, &p, &lp) == ZRT_OK && lp.lds_bytes <= (160u << 10), "%s launch plan: %s", nm, zrt_last_error());
        if (!bvh || !use_bvh) CHECK(lp.sampling_loop == 0 || lp.sampling_loop == 6, "%s: not a list loop (%u)", nm, lp.sampling_loop);
      }
    if (bvh) {
      const int rc = zrt_debug_qnodes(s, &n_slots);
      if (name == "inf-vertex")
        CHECK(rc == ZRT_E_UNSUPPORTED && std::strstr(zrt_last_error(), "refused"), "%s qnodes: rc %d %s", nm, rc, zrt_last_error());
      else
        CHECK(rc == ZRT_OK && n_slots > 0, "%s qnodes: %s", nm, zrt_last_error());
      // a launch that asks for compressed nodes gets them, or (a refused tree) the full ones
      setenv("ZRT_QNODES", "1", 1);
      setenv("ZRT_POOL", "1", 1);
      p = params(24, 24, 4, 6, ZRT_RNG_COUNTER);
      CHECK(zrt_debug_launch_plan(s, &p, &lp) == ZRT_OK && lp.sampling_loop == 5 && lp.qnodes == (name == "inf-vertex" ? 0u : 1u),
            "%s: launch plan under ZRT_QNODES=1: loop %u qnodes %u", nm, lp.sampling_loop, lp.qnodes);
      unsetenv("ZRT_QNODES");
      unsetenv("ZRT_POOL");
    }
  }

  // the oracle's closest hits through the BVH and through the list
  const uint32_t n = 6000;
  const std::vector<float> rays = rays_of(f, n);
  std::vector<float> t(n);
  std::vector<int32_t> pb(n, -1), pl(n, -1);
  CHECK(oracle_trace(s, 0, rays.data(), n, t.data(), pl.data()) == 0, "%s: oracle_trace (list)", nm);
  if (bvh) CHECK(oracle_trace(s, 1, rays.data(), n, t.data(), pb.data()) == 0, "%s: oracle_trace (bvh)", nm);
  uint32_t hits_b = 0, hits_l = 0, flat_b = 0, flat_l = 0, marked_wins = 0;
  std::vector<int32_t> wb, wl;
  for (uint32_t i = 0; i < n; ++i) {
    hits_b += pb[i] >= 0, hits_l += pl[i] >= 0;
    flat_b += is_marked(f, pb[i]), flat_l += is_marked(f, pl[i]);
    marked_wins += is_marked(f, pb[i]) || is_marked(f, pl[i]);
    if (pb[i] >= 0 && std::find(wb.begin(), wb.end(), pb[i]) == wb.end()) wb.push_back(pb[i]);
    if (pl[i] >= 0 && std::find(wl.begin(), wl.end(), pl[i]) == wl.end()) wl.push_back(pl[i]);
  }
  std::sort(wb.begin(), wb.end());
  std::sort(wl.begin(), wl.end());
  std::printf("degenerate %s: %u primitives, %u of %u leaves flat, %u BVH hits and %u list hits of %u rays (%u and %u on marked)\n", nm,
              sc.n_prims, n_flat, n_leaves, hits_b, hits_l, n, flat_b, flat_l);
  if (f.flat_axis >= 0)
    CHECK(hits_b == 0 && 4 * hits_l >= n && n_flat == n_leaves, "%s: %u BVH hits, %u list hits, %u of %u leaves flat", nm, hits_b,
          hits_l, n_flat, n_leaves);
  else if (name == "terraces")
    CHECK(n_flat >= 20 && n_flat < n_leaves && flat_l - flat_b >= 1000, "%s: %u flat leaves, %u - %u hits on flat triangles", nm,
          n_flat, flat_l, flat_b);
  else if (name == "duplicates")
    CHECK(wb != wl && wb.size() == 2 && wl.size() == 2, "%s: the BVH's winners are the list's", nm);
  else if (name == "points" || name == "slivers" || name == "range" || name == "eleven")
    CHECK(5 * hits_b >= n, "%s: %u BVH hits of %u rays", nm, hits_b, n);
  if (name == "slivers") CHECK(marked_wins == 0, "%s: %u rays won by a sliver", nm, marked_wins);
}

static void all() {
  for (const char* name : {"eleven", "ten", "flat-x", "flat-y", "flat-z", "terraces", "duplicates", "points", "slivers", "range",
                           "inf-vertex", "inf-radius", "nan-vertex", "nan-center"})
    one_family(name);
}

}  // namespace degenerate

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s ASSETS_DIR TMP_DIR\n", argv[0]);
    return 2;
  }
  const std::string assets = argv[1], tmp = argv[2];
  for (uint32_t i : {0u, 1u, 2u, 3u, 4u}) one_scene(i, assets, tmp);
  pass_and_adapt_plans();
  radiance_plans();
  camera_plans();
  reproject_plans(assets);
  tile_walks();
  degenerate::all();

  // error paths: unknown scene index, missing files, a truncated binary scene
  zrt_scene_data* d = nullptr;
  zrt_camera cam;
  CHECK(zrt_scene_load(99, assets.c_str(), &d, &cam) == ZRT_E_INVALID, "scene 99 accepted");
  CHECK(zrt_scene_read((tmp + "/missing.zrts").c_str(), &d, &cam) != ZRT_OK, "missing scene file accepted");
  {
    const std::string trunc = tmp + "/trunc.zrts";
    FILE* in = std::fopen((tmp + "/scene2.zrts").c_str(), "rb");
    FILE* out = std::fopen(trunc.c_str(), "wb");
    if (in && out) {
      std::vector<char> buf(4096);
      const size_t n = std::fread(buf.data(), 1, buf.size(), in);
      std::fwrite(buf.data(), 1, n / 2, out);
    }
    if (in) std::fclose(in);
    if (out) std::fclose(out);
    CHECK(zrt_scene_read(trunc.c_str(), &d, &cam) != ZRT_OK, "truncated scene file accepted");
  }
  zrt_prim* prims = nullptr;
  uint32_t n = 0;
  CHECK(zrt_obj_read((tmp + "/missing.obj").c_str(), 0, &prims, &n) != ZRT_OK, "missing OBJ accepted");
  CHECK(zrt_obj_read((assets + "/teapot.obj").c_str(), 0, &prims, &n) == ZRT_OK && n > 6000, "teapot.obj: %s",
        zrt_last_error());
  zrt_free(prims);

  // PNG codec: the reference's textures in, PNG / PPM out, read back
  for (const char* name : {"earthmap.png", "nitor-logo-25.png"}) {
    uint32_t w = 0, h = 0;
    float* px = nullptr;
    int rc = zrt_image_read_png((assets + "/" + name).c_str(), &w, &h, &px);
    CHECK(rc == ZRT_OK && w > 0 && h > 0, "%s: %s", name, zrt_last_error());
    if (rc) continue;
    const std::string png = tmp + "/out.png", ppm = tmp + "/out.ppm";
    CHECK(zrt_image_write_png(png.c_str(), px, w, h) == ZRT_OK, "write png: %s", zrt_last_error());
    CHECK(zrt_image_write_ppm(ppm.c_str(), px, w, h) == ZRT_OK, "write ppm: %s", zrt_last_error());
    uint32_t w2 = 0, h2 = 0;
    float* back = nullptr;
    CHECK(zrt_image_read_png(png.c_str(), &w2, &h2, &back) == ZRT_OK && w2 == w && h2 == h &&
              std::memcmp(back, px, sizeof(float) * 3 * w * h) == 0,
          "%s: PNG round trip differs", name);
    zrt_free(back);
    zrt_free(px);
  }
  uint32_t w = 0, h = 0;
  float* px = nullptr;
  CHECK(zrt_image_read_png((assets + "/teapot.obj").c_str(), &w, &h, &px) != ZRT_OK, "an OBJ decoded as PNG");

  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("sanitized host run ok\n");
  return 0;
}
