// flatten.cpp - the scene flattened for the device: the reference BVH in
// pre-order, the wide tree (accel_build) in the layout the kernels decode,
// primitive slots in DFS leaf order, materials and texels.  No HIP call: the
// device BVH build is bvh_gpu.hip's.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "accel_build.hpp"
#include "bvh_build.hpp"
#include "host.hpp"

namespace zrt {
namespace {
const KernelConfig& K = kernel_config();

// Meshes from this many primitives have their reference BVH built on the GPU
// (bvh_gpu.hip: same tree; 1.6 M triangles in a fraction of a second instead of
// 5.6 s on the host).  ZRT_BVH_DEVICE=0/1 forces the host / device build.
constexpr uint32_t kDeviceBvhMin = 1u << 16;
bool device_bvh(uint32_t n) {
  if (const char* e = std::getenv("ZRT_BVH_DEVICE")) return std::atoi(e) != 0;
  return n >= kDeviceBvhMin;
}

// The grazing margins' coefficient (DESIGN.md §3 "Grazing rays"): 2^-18;
// ZRT_GRAZE_M overrides it (A/B of larger margins)
float graze_margin() {
  if (const char* e = std::getenv("ZRT_GRAZE_M")) return std::max(0x1p-18f, float(std::atof(e)));
  return 0x1p-18f;
}

// The grazing-triangle guard's coefficient for a scene (DESIGN.md §3
// "Triangles"): an accepted hit of the rounded test (triangle.zig:48-70) lies
// outside its triangle by at most K u |ao| |e1||e2| / det, K = 2.6 the largest
// measured (tools/tri_reach.py; 1.3 on the reference scenes' own triangles,
// tools/tri_reach_bound.py gives the first-order worst case), and det >= 1e-6:
// K u max |e1||e2| / 1e-6 per unit of |ao| <= T + extent (guard_grow).  Capped at
// 2^-10 (above it the guard opens much of the tree; the teapot's model asks 0.024):
// the grazing-triangle rays of every reference scene are exact from 2^-12
// (profiles/r04/r04f).  ZRT_GUARD_K overrides it (A/B).
float guard_model(double max_p12) {
  if (const char* e = std::getenv("ZRT_GUARD_K")) return std::max(0.0f, float(std::atof(e)));
  const double k = 2.6 * 0x1p-24 * max_p12 / 1e-6;
  return float(std::min(k, double(0x1p-10)));
}
}  // namespace

// Flatten the scene for the device: BVH (pre-order), slots in DFS leaf order.
// `device` >= 0: the GPU that may build the BVH (device_bvh).  `qnodes`: build
// the compressed nodes too (1), not (0), or as want_qnodes decides (-1, ZRT_QNODES).
void flatten_scene(HostScene* c, const zrt_scene* s, bool use_bvh, int device, int qnodes) {
  const double t0 = now_ms();
  const uint32_t n = s->n_prims;
  std::vector<uint32_t> slot_to_prim, leaf_of_slot;
  std::vector<float4> nodes;
  uint32_t depth = 0;
  if (use_bvh) {
    BuiltBvh bvh;
    bool built = false;
    if (device >= 0 && device_bvh(n)) {
      // the same tree on the GPU; any HIP failure there (hipMalloc on a busy GPU,
      // a hipcub error) falls back to the host build, which gives the same tree
      try {
        built = build_bvh_device(s->prims, n, device, &bvh);
      } catch (const Error& e) {
        if (std::getenv("ZRT_DEBUG_LAUNCH"))
          std::fprintf(stderr, "zrt preprocess: device BVH build failed (%s); host build\n", e.what());
        c->device_bvh_failed = true;  // (flatten_for_device clears the failed build's sticky runtime error)
      }
    }
    if (!built) bvh = build_bvh(s->prims, n);
    if (std::getenv("ZRT_DEBUG_LAUNCH"))
      std::fprintf(stderr, "zrt preprocess: reference BVH %zu nodes in %.1f ms\n", bvh.nodes.size(), now_ms() - t0);
    depth = bvh.max_depth;
    nodes.resize(2 * bvh.nodes.size());
    std::vector<int32_t> prim_slot(n, -1);
    auto ref_of = [&](int32_t child) -> int32_t {
      if (child >= 0) return child;
      const uint32_t prim = uint32_t(-child - 1);
      if (prim_slot[prim] < 0) {
        prim_slot[prim] = int32_t(slot_to_prim.size());
        slot_to_prim.push_back(prim);
      }
      const int32_t kind = s->prims[prim].kind == ZRT_PRIM_TRIANGLE ? 1 : 0;
      return -(2 * prim_slot[prim] + kind) - 1;
    };
    std::vector<RefLeaf> leaves;
    for (size_t i = 0; i < bvh.nodes.size(); ++i) {  // pre-order == reference DFS order
      const BuildNode& b = bvh.nodes[i];
      const int32_t l = ref_of(b.left);
      const int32_t r = ref_of(b.right);
      if (b.left < 0) {  // a reference leaf: its box and its primitive refs
        for (const int32_t ref : {l, r}) {
          const uint32_t slot = uint32_t(-ref - 1) >> 1;
          if (leaf_of_slot.size() <= slot) leaf_of_slot.resize(slot + 1);
          leaf_of_slot[slot] = uint32_t(i);
        }
        RefLeaf L;
        for (int k = 0; k < 3; ++k) {
          L.mn[k] = b.mn[k];
          L.mx[k] = b.mx[k];
        }
        L.prim_a = l;
        L.prim_b = r;
        leaves.push_back(L);
      }
      float4 lo, hi;
      lo.x = b.mn[0]; lo.y = b.mn[1]; lo.z = b.mn[2];
      hi.x = b.mx[0]; hi.y = b.mx[1]; hi.z = b.mx[2];
      std::memcpy(&lo.w, &l, 4);
      std::memcpy(&hi.w, &r, 4);
      nodes[2 * i] = lo;
      nodes[2 * i + 1] = hi;
    }
    c->n_nodes = uint32_t(bvh.nodes.size());
    // Spheres (DESIGN.md §3 "Spheres").  The rounded disc of sphere.zig:31-41 errs by
    // E <= 32 u (|oc|^2 + r^2) (u = 2^-24, three rounded dot products and two
    // subtractions), so an accepted ray passes within sqrt(r^2 + E) - r <= sqrt(E) of
    // the sphere and its hit errs by <= 1.5 sqrt(E) in t: subtrees holding a sphere
    // are grown by 2 sqrt(E) = 2^-8.5 R, R >= |oc| + r for every ray whose origin
    // lies within 2 H of the root box's center on every axis (H: its largest half
    // extent; |oc| <= 2 sqrt(3) H + sqrt(3) H, r <= H).  Rays from farther out are
    // traced the reference's way (render.hip ray_origin_ok).
    c->ref_sph.assign(bvh.nodes.size(), 0);
    bool any_sphere = false;
    for (size_t i = bvh.nodes.size(); i-- > 0;) {  // pre-order: children after their parent
      const BuildNode& b = bvh.nodes[i];
      uint8_t f = 0;
      for (const int32_t ch : {b.left, b.right}) {
        if (ch >= 0) f |= c->ref_sph[size_t(ch)];
        else f |= s->prims[uint32_t(-ch - 1)].kind == ZRT_PRIM_SPHERE ? 1 : 0;
      }
      c->ref_sph[i] = f;
      any_sphere = any_sphere || f;
    }
    // The region the bound is sized over: the root box united with every sphere's
    // centre -+ |radius|.  A negative radius (the reference scenes use them) makes
    // sphere.zig:25's box inverted, so the root box alone need not cover that
    // sphere's surface.
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
      lo[k] = bvh.nodes[0].mn[k];
      hi[k] = bvh.nodes[0].mx[k];
    }
    for (uint32_t i = 0; i < n; ++i) {
      const zrt_prim& p = s->prims[i];
      if (p.kind != ZRT_PRIM_SPHERE) continue;
      const float r = std::fabs(p.radius), cc[3] = {p.center.x, p.center.y, p.center.z};
      for (int k = 0; k < 3; ++k) {  // (rounded outward: the f32 box contains the exact one)
        lo[k] = std::min(lo[k], std::nextafter(cc[k] - r, -HUGE_VALF));
        hi[k] = std::max(hi[k], std::nextafter(cc[k] + r, HUGE_VALF));
      }
    }
    float H = 0.0f;
    for (int k = 0; k < 3; ++k) {
      c->root_c[k] = 0.5f * lo[k] + 0.5f * hi[k];
      H = std::max(H, std::max(hi[k] - c->root_c[k], c->root_c[k] - lo[k]));
    }
    if (!(H < 0x1p100f)) H = 0x1p100f;  // NaN / huge extents: every origin fails ray_origin_ok's bound
    // Only sphere slots depend on where a ray starts (their growth is sized for
    // origins within 2 H); the triangle margins do not, so a scene without spheres
    // accepts every origin (a distant camera no longer replays every ray)
    c->origin_bound = any_sphere ? 2.0f * H : HUGE_VALF;
    const float sphere_grow = any_sphere ? float(std::ldexp(std::sqrt(2.0), -9) * (3.0 * std::sqrt(3.0) + 1.0) * double(H)) : 0.0f;
    const double tw = now_ms();
    c->graze_m = graze_margin();
    c->graze_leaf = std::max(c->graze_m, 0x1p-18f);  // (KArgs::graze_leaf: no kernel reads it)
    c->guard = 0.0f;  // (set below, once the triangles are known)
    // the top levels stored first (LDS): two for the full 128-B nodes; a tree that
    // also gets compressed nodes stores qtop_levels() (their 64-B nodes leave room
    // for a third level in the path pool's LDS), the full kernels reading the first two
    const uint32_t n_leaf_est = uint32_t(leaves.size());
    const bool want_q = qnodes >= 0 ? qnodes != 0 : want_qnodes((n_leaf_est + 2) / 3);  // (about leaves / 3 nodes)
    const uint32_t top_levels = want_q ? qtop_levels() : 2u;
    const WideBvh wide = build_wide_bvh(leaves, top_levels, 0.5f * c->graze_m, sphere_grow, true);
    if (std::getenv("ZRT_DEBUG_LAUNCH"))
      std::fprintf(stderr, "zrt preprocess: wide tree %u nodes in %.1f ms\n", wide.n_nodes, now_ms() - tw);
    const size_t nw = wide.nodes.size();
    // one copy per ray octant o (bit k set: direction k negative) with axis k's
    // min / max planes swapped, so float4 0-2 are the near planes, 3-5 the far
    std::vector<float4> wn(K.oct_copies * nw);
    for (uint32_t o = 0; o < K.oct_copies; ++o) {
      float4* dst = wn.data() + o * nw;
      std::memcpy(dst, wide.nodes.data(), nw * sizeof(float4));
      for (size_t i = 0; i < nw; i += 8)
        for (int k = 0; k < 3; ++k)
          if (o >> k & 1u) std::swap(dst[i + k], dst[i + 3 + k]);
    }
    c->wide_stack = wide.max_stack + 3;  // + the dead entries of a branch-free push
    // compressed nodes for trees past the caches (want_qnodes): the same tree, 64-B nodes
    // (quantize_wide stores octant copies with pre-swapped planes, which wide_iter_q
    // reads as such)
    if (want_q) {
      const double tq = now_ms();
      QuantWide qw = quantize_wide(wide);
      if (qw.ok) {
        c->qn.resize(qw.nodes.size());
        std::memcpy(c->qn.data(), qw.nodes.data(), qw.nodes.size() * sizeof(float4));
        c->ql.resize(std::max<size_t>(1, qw.leaves.size()));
        std::memcpy(c->ql.data(), qw.leaves.data(), qw.leaves.size() * sizeof(float4));
        c->q_ok = true;
        c->q_stride = qw.n_nodes * kQuantNodeF4;
        c->q_top = wide.n_top;
      }
      if (std::getenv("ZRT_DEBUG_LAUNCH"))
        std::fprintf(stderr, "zrt preprocess: compressed nodes %s, %u leaf records, %.1f ms\n", qw.ok ? "built" : "refused",
                     qw.n_leaves, now_ms() - tq);
    }
    c->wn = std::move(wn);
    c->wide_stride = uint32_t(nw);
    c->n_wide = wide.n_nodes;
    c->n_leaves = wide.n_leaves;
    c->n_top = wide.level_end.empty() ? 0u : wide.level_end[std::min<size_t>(2, wide.level_end.size()) - 1];
    // (either node format's octant offsets within the kernels' multiply)
    check_octant_offsets(uint32_t(std::min<size_t>(nw, 0xffffffffu)), c->n_top, 8u);
    if (c->q_ok) check_octant_offsets(c->q_stride, c->q_top, kQuantNodeF4);
    c->layout = wide.layout;
    if (const char* e = std::getenv("ZRT_DEBUG_TREE_LAYOUT"))  // tests: a tree another kernel would have to decode
      c->layout ^= uint32_t(std::strtoul(e, nullptr, 0));
    if (c->layout != K.layout)
      throw Error(ZRT_E_UNSUPPORTED, "the wide tree's layout (" + std::to_string(c->layout) +
                                         ") is not the one this library's kernels decode (" +
                                         std::to_string(K.layout) + "): accel_build and render.hip disagree");
  } else {
    for (uint32_t i = 0; i < n; ++i) slot_to_prim.push_back(i);
  }
  std::vector<float4> prims(3 * size_t(slot_to_prim.size()));
  std::vector<float4> shade(slot_to_prim.size());
  double tlo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, thi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  double tri_p12 = 0.0;  // the largest |e1| |e2| (guard_model)
  for (size_t sl = 0; sl < slot_to_prim.size(); ++sl) {
    const zrt_prim& p = s->prims[slot_to_prim[sl]];
    if (p.kind == ZRT_PRIM_TRIANGLE)  // ray_slack: the triangles' largest |coordinate|
      for (const auto& v : {p.a, p.b, p.c}) {
        c->scene_extent = std::max({c->scene_extent, std::fabs(v.x), std::fabs(v.y), std::fabs(v.z)});
        const double vk[3] = {v.x, v.y, v.z};
        for (int k = 0; k < 3; ++k) {  // (NaN coordinates: the box becomes NaN, paxis_grow infinite)
          tlo[k] = vk[k] < tlo[k] || vk[k] != vk[k] ? vk[k] : tlo[k];
          thi[k] = vk[k] > thi[k] || vk[k] != vk[k] ? vk[k] : thi[k];
        }
      }
    float4* q = &prims[3 * sl];
    float4& sh = shade[sl];
    uint32_t tag = p.material;
    if (p.kind == ZRT_PRIM_TRIANGLE) {
      // triangle.zig:35-38: e1 = b-a, e2 = c-a, n = e1 x e2, unit n = n / |n|
      const float e1x = p.b.x - p.a.x, e1y = p.b.y - p.a.y, e1z = p.b.z - p.a.z;
      const float e2x = p.c.x - p.a.x, e2y = p.c.y - p.a.y, e2z = p.c.z - p.a.z;
      const float nx = e1y * e2z - e1z * e2y;
      const float ny = e1z * e2x - e1x * e2z;
      const float nz = e1x * e2y - e1y * e2x;
      const float len = std::sqrt(nx * nx + ny * ny + nz * nz);
      q[0] = make_float4(p.a.x, p.a.y, p.a.z, e1x);
      q[1] = make_float4(e1y, e1z, e2x, e2y);
      q[2] = make_float4(e2z, nx, ny, nz);
      tag |= 0x80000000u;
      sh = make_float4(nx / len, ny / len, nz / len, 0.0f);
      // |det| = |d . n| <= |d| |n| < (1 + 2^-22) sqrt(3) 2^124 < 2^126 (NaN fails too)
      const float mn = std::max(std::fabs(nx), std::max(std::fabs(ny), std::fabs(nz)));
      if (!(mn < 0x1p124f)) c->tri_rcp_fast = 0;
      // the grazing guard's model (guard_model): the largest |e1| |e2| of the scene
      const double p12 = std::sqrt((double(e1x) * e1x + double(e1y) * e1y + double(e1z) * e1z) *
                                   (double(e2x) * e2x + double(e2y) * e2y + double(e2z) * e2z));
      if (p12 == p12) tri_p12 = std::max(tri_p12, p12);
    } else {
      q[0] = make_float4(p.center.x, p.center.y, p.center.z, p.radius * p.radius);  // sphere.zig:35 r*r, once
      q[1] = make_float4(0, 0, 0, 0);
      q[2] = make_float4(0, 0, 0, 0);
      sh = make_float4(1.0f / p.radius, 0.0f, 0.0f, 0.0f);  // sphere.zig:46 scale(1.0/radius)
    }
    std::memcpy(&sh.w, &tag, 4);
  }
  if (use_bvh) c->guard = guard_model(tri_p12);
  // the triangles' bounding box as centre and half extents, rounded so that the
  // f32 box contains the exact one (paxis_grow); no triangle: an empty box at 0
  for (int k = 0; k < 3; ++k) {
    if (!(tlo[k] <= thi[k])) {
      if (tlo[k] == HUGE_VAL) tlo[k] = thi[k] = 0.0;  // no triangles
      else { c->tri_c[k] = 0.0f; c->tri_h[k] = HUGE_VALF; continue; }  // NaN
    }
    const double ctr = 0.5 * tlo[k] + 0.5 * thi[k];
    c->tri_c[k] = float(ctr);
    const double h = std::max(thi[k] - double(c->tri_c[k]), double(c->tri_c[k]) - tlo[k]);
    c->tri_h[k] = std::nextafter(float(h), HUGE_VALF);
  }
  // materials + textures.  An image whose every value is exactly k/255 (what
  // png_image.zig:76-89 produces) is stored as 8-bit RGBX and expanded through
  // a table of the same f32 values; any other image stays f32 RGB.
  float lut[256];
  for (int k = 0; k < 256; ++k) lut[k] = float(k) / 255.0f;
  std::vector<DevMaterial> mats(s->n_materials);
  std::vector<uint64_t> img_off(s->n_images);
  std::vector<uint32_t> img_u8(s->n_images, 0);
  uint64_t texel_count = 0, texel8_count = 0;
  for (uint32_t i = 0; i < s->n_images; ++i) {
    const zrt_image& im = s->images[i];
    const size_t nv = 3 * size_t(im.width) * im.height;
    bool exact = true;
    for (size_t j = 0; j < nv && exact; ++j) {
      const float v = im.pixels[j];
      const long k = std::lrint(double(v) * 255.0);
      exact = k >= 0 && k <= 255 && std::memcmp(&lut[k], &v, 4) == 0;
    }
    img_u8[i] = exact ? 1u : 0u;
    uint64_t& count = exact ? texel8_count : texel_count;
    img_off[i] = count;
    count += uint64_t(im.width) * im.height;
  }
  if (texel_count >= (1ull << 30) || texel8_count >= (1ull << 30))  // (att codes carry a 30-bit texel index)
    throw Error(ZRT_E_UNSUPPORTED, "more than 2^30 texels in one store");
  for (uint32_t i = 0; i < s->n_materials; ++i) {
    const zrt_material& m = s->materials[i];
    DevMaterial dm{};
    dm.kind = m.kind;
    dm.ior = m.index_of_refraction;
    dm.tex_kind = ZRT_TEX_COLOR;
    // (the kernels take every kind that is neither Lambertian nor metal as a dielectric)
    if (m.kind != ZRT_MAT_LAMBERTIAN && m.kind != ZRT_MAT_METAL) c->has_dielectric = 1;
    if (m.kind != ZRT_MAT_DIELECTRIC) {
      const zrt_texture& t = s->textures[m.texture];
      dm.tex_kind = t.kind;
      if (t.kind != ZRT_TEX_COLOR) c->has_image_texture = 1;
      dm.r = t.color.x;
      dm.g = t.color.y;
      dm.b = t.color.z;
      dm.u_off = t.u_offset;
      dm.v_off = t.v_offset;
      if (t.kind == ZRT_TEX_IMAGE) {
        dm.img_w = s->images[t.image].width;
        dm.img_h = s->images[t.image].height;
        dm.img_off = uint32_t(img_off[t.image]);
        dm.img_u8 = img_u8[t.image];
      }
    }
    mats[i] = dm;
  }
  std::vector<float> tex(3 * texel_count);
  std::vector<uint32_t> tex8(texel8_count);
  for (uint32_t i = 0; i < s->n_images; ++i) {
    const zrt_image& im = s->images[i];
    const size_t np = size_t(im.width) * im.height;
    if (img_u8[i]) {
      for (size_t j = 0; j < np; ++j) {
        uint32_t px = 0;
        for (int ch = 0; ch < 3; ++ch)
          px |= uint32_t(std::lrint(double(im.pixels[3 * j + ch]) * 255.0)) << (8 * ch);
        tex8[img_off[i] + j] = px;
      }
    } else {
      std::memcpy(&tex[3 * img_off[i]], im.pixels, sizeof(float) * 3 * np);
    }
  }
  c->texel_bytes = s->n_images == 0 ? 0u : texel_count == 0 ? 4u : 12u;
  c->nodes = std::move(nodes);
  c->prims = std::move(prims);
  c->shade = std::move(shade);
  c->mats = std::move(mats);
  c->tex = std::move(tex);
  c->tex8 = std::move(tex8);
  c->slot_to_prim = std::move(slot_to_prim);
  c->leaf_of_slot = std::move(leaf_of_slot);
  c->preprocess_ms = now_ms() - t0;
  c->use_bvh = use_bvh;
  c->n_prims = n;
  c->bvh_depth = depth;
}

SceneShape shape_of(const HostScene& h) {  // (as upload_scene fills the context)
  SceneShape s;
  s.tri_rcp_fast = h.tri_rcp_fast != 0;
  s.has_dielectric = h.has_dielectric != 0;
  s.has_image_texture = h.has_image_texture != 0;
  s.use_bvh = h.use_bvh;
  s.q_ok = h.q_ok;
  s.n_nodes = h.n_nodes;
  s.n_wide = h.n_wide;
  s.wide_stack = h.wide_stack;
  s.stack_depth = h.use_bvh ? h.bvh_depth + 2 : 0;
  s.n_top = h.n_top;
  s.q_top = h.q_top;
  s.n_mats = uint32_t(h.mats.size());
  s.guard = h.guard;
  return s;
}
}  // namespace zrt
