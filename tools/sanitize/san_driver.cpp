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
//   oracle/        oracle_render (both RNG modes), oracle_render_scanlines,
//                  oracle_trace, oracle_bvh_build
//
// Device code is not built here (GPU sanitizers are not available on the pool);
// build_bvh_device is stubbed to "not available", which is what the host build
// path does without a GPU, and kernel_config() (render.hip's) returns the values the
// shipped kernels are built with.  Any sanitizer report aborts with a non-zero status
// (-fno-sanitize-recover=all); tests/test_sanitizers.py builds and runs this.
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
    c.lds_top = c.lane_lds = c.mats_lds_only = c.lean_default = c.grow = c.sphere_slots = true;
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

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s ASSETS_DIR TMP_DIR\n", argv[0]);
    return 2;
  }
  const std::string assets = argv[1], tmp = argv[2];
  for (uint32_t i : {0u, 1u, 2u, 3u, 4u}) one_scene(i, assets, tmp);
  pass_and_adapt_plans();
  reproject_plans(assets);
  tile_walks();

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
