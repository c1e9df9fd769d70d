// tile_class.cpp - the conservative tile classifier: which 8x8 tiles of a frame are
// all sky, i.e. no primary ray the kernels can generate for any of their pixels can
// return a hit from the reference's closest-hit query (DESIGN.md §3 "All-sky tiles").
// Such tiles render in sky_kernel (render.hip) with no traversal.  And which are
// one-sphere(s): no such ray can return a hit from any primitive but the sphere s
// (DESIGN.md §3 "One-sphere tiles"); their camera rays test s alone, without walking the
// tree (render.hip render_loop ONE_SPHERE).  Pure host C++:
// no HIP call; the host sanitizer program links and drives it (tools/sanitize).
//
// The proof, per block of tiles: every ray of the block leaves the camera origin
// inside a cone (axis, half-angle: from the block's jitter footprint, computed in
// double, widened for the f32 rounding of Camera.getRay).  A primitive test accepts
// a ray only if the ray's line passes within the primitive's reach of it, so the
// block is sky when the cone misses the bounding sphere, grown by that reach, of
// every box of the reference tree it cannot cull.  Anything undecided is general.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "host.hpp"

namespace zrt {
static_assert(kTileSky == ZRT_TILE_SKY && kTileOneSphere == ZRT_TILE_ONE_SPHERE, "zrt.h names the class words");
namespace {
constexpr double kU = 0x1p-24;
constexpr uint32_t kMaxSkyNodes = 1u << 21;  // larger trees are not kept for classification (all general)
constexpr uint32_t kTileBudget = 512;        // bounding-sphere tests one tile may spend; past it: general
constexpr uint32_t kBlockBudget = 4096;      // ... one block of tiles, past it the rest is handed down unrefined

struct V {
  double x, y, z;
};
inline V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V operator*(V a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double len(V a) { return std::sqrt(dot(a, a)); }
inline V vec(const zrt_vec3& v) { return {double(v.x), double(v.y), double(v.z)}; }
inline bool finite3(V a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }

// The rays of a block of tiles: directions within `angle` of the unit axis, as (cos, sin).
struct Cone {
  V axis;
  double c, s;
  bool ok;
};

struct Classifier {
  const SkyScene& S;
  V o, llc, hor, ver;
  double W, H;           // width, height (the jitter's divisors)
  uint32_t xbound, height, tiles_x, tiles_y, rank, world;
  double eps;            // angular slack of a generated direction against the exact one
  double reach_tri, reach_inner;  // triangles' reach; the largest reach of any primitive (inner boxes)
  std::vector<double> sphere_r;   // per sphere (S.spheres order): its radius grown by its reach
  std::vector<uint32_t>* cls;
  uint32_t n_sky = 0;
  bool want_one = false;          // mark one-sphere tiles too
  std::vector<uint32_t> n_one;    // per sphere (S.spheres order): the tiles marked one-sphere(it)
  std::vector<std::vector<int32_t>> frontier;  // per recursion depth
  std::vector<int32_t> stack;

  Cone cone_of(uint32_t tx0, uint32_t ty0, uint32_t tx1, uint32_t ty1) const {
    // px + r - 0.5 with r in [0, 1), rounded: within [px - 0.5, px + 0.5]
    const double x_lo = double(tx0 * 8u) - 0.5, x_hi = double(std::min(tx1 * 8u, xbound) - 1u) + 0.5;
    const double y_lo = double(ty0 * 8u) - 0.5, y_hi = double(std::min(ty1 * 8u, height) - 1u) + 0.5;
    const double us[2] = {x_lo / W, x_hi / W}, vs[2] = {y_lo / H, y_hi / H};
    V d[4], sum{0, 0, 0};
    for (int i = 0; i < 4; ++i) {
      const V p = llc + hor * us[i & 1] + ver * vs[i >> 1] - o;
      const double l = len(p);
      if (!(l > 0.0)) return Cone{{0, 0, 1}, 0, 1, false};
      d[i] = p * (1.0 / l);
      sum = sum + d[i];
    }
    const double ls = len(sum);
    if (!(ls > 1e-3)) return Cone{{0, 0, 1}, 0, 1, false};
    Cone k;
    k.axis = sum * (1.0 / ls);
    // the angle to the axis over a planar convex footprint is largest at a corner
    // (its sublevel sets are conic sections: convex while the angle stays below 90 degrees)
    double c = 1.0;
    for (int i = 0; i < 4; ++i) c = std::min(c, dot(k.axis, d[i]));
    const double s = std::sqrt(std::max(0.0, 1.0 - c * c));
    k.c = c - eps * s - eps * eps - 1e-12;  // <= cos(angle + eps)
    k.ok = k.c > 0.1;
    k.s = std::sqrt(std::max(0.0, 1.0 - k.c * k.c));
    return k;
  }
  // Can a ray of the cone pass within R of the point c?  (false: proved not)
  bool touches(const Cone& k, V c, double R) const {
    const V w = c - o;
    const double d2 = dot(w, w);
    if (!(d2 > R * R)) return true;
    const double dist = std::sqrt(d2), sa = R / dist, ca = std::sqrt(1.0 - sa * sa);
    // the ray's angle to w is at least phi - angle; it misses iff that exceeds asin(R / dist)
    return !(dot(k.axis, w) / dist < k.c * ca - k.s * sa - 1e-12);
  }
  // Does every ray of the cone run into one sphere (shrunk a little)?  Then the block is
  // general whatever else it sees: no need to split it further.  (A shortcut only:
  // general is always a safe answer.)
  // Returns that sphere's index (S.spheres order), or -1.
  int32_t inside_a_sphere(const Cone& k) const {
    if (S.spheres.size() > 16) return -1;
    for (size_t i = 0; i < S.spheres.size(); ++i) {
      const SkyPrim& q = S.prims[S.spheres[i]];
      const V w = V{q.c[0], q.c[1], q.c[2]} - o;
      const double dist = len(w), r = 0.999 * q.r;
      if (!(dist > r)) continue;
      const double sa = r / dist, ca = std::sqrt(1.0 - sa * sa);
      if (sa > k.s && dot(k.axis, w) / dist > ca * k.c + sa * k.s) return int32_t(i);
    }
    return -1;
  }
  // The one sphere (its index) a frontier of touched boxes and primitives reduces to:
  // every entry is that sphere's primitive, and its leaf is one the one-sphere path can
  // stand in for (SkyScene::sphere_root).  -1: anything else.
  int32_t sole_sphere(const std::vector<int32_t>& f) const {
    int32_t one = -1;
    for (const int32_t n : f) {
      if (n >= 0) return -1;
      const int32_t si = S.prims[uint32_t(-n - 1) >> 1].sphere_index;
      if (si < 0 || !S.sphere_root[size_t(si)] || (one >= 0 && one != si)) return -1;
      one = si;
    }
    return one;
  }
  bool prim_touches(const Cone& k, int32_t ref) const {
    const SkyPrim& p = S.prims[uint32_t(-ref - 1) >> 1];
    if (p.sphere_index >= 0) return touches(k, V{p.c[0], p.c[1], p.c[2]}, sphere_r[size_t(p.sphere_index)]);
    if (p.r < 0.0) return false;  // a triangle no ray can hit (|n| below the reference's det floor)
    return touches(k, V{p.c[0], p.c[1], p.c[2]}, p.r + reach_tri);
  }

  // one < 0: sky; else one-sphere(sphere index `one`)
  void mark(uint32_t tx0, uint32_t ty0, uint32_t tx1, uint32_t ty1, int32_t one = -1) {
    for (uint32_t ty = ty0; ty < ty1; ++ty)
      for (uint32_t tx = tx0; tx < tx1; ++tx) {
        const uint32_t t = ty * tiles_x + tx;
        if (t % world != rank) continue;
        if (one < 0) {
          (*cls)[t / world] = kTileSky;
          ++n_sky;
        } else {
          (*cls)[t / world] = kTileOneSphere | S.spheres[size_t(one)];
          ++n_one[size_t(one)];
        }
      }
  }
  bool owns_any(uint32_t tx0, uint32_t ty0, uint32_t tx1, uint32_t ty1) const {
    if (world == 1 || tx1 - tx0 >= world) return true;  // (a row's run of `world` tiles holds every rank's)
    for (uint32_t ty = ty0; ty < ty1; ++ty)
      for (uint32_t tx = tx0; tx < tx1; ++tx)
        if ((ty * tiles_x + tx) % world == rank) return true;
    return false;
  }

  void block(uint32_t tx0, uint32_t ty0, uint32_t tx1, uint32_t ty1, size_t depth) {
    if (!owns_any(tx0, ty0, tx1, ty1)) return;
    const bool single = tx1 - tx0 == 1 && ty1 - ty0 == 1;
    const Cone k = cone_of(tx0, ty0, tx1, ty1);
    if (depth + 1 >= frontier.size()) return;  // (never: a split halves the block)
    const std::vector<int32_t>& in = frontier[depth];
    std::vector<int32_t>& out = frontier[depth + 1];
    out.clear();
    int32_t inside = -1;  // the sphere every ray of the cone runs into
    if (!k.ok) {
      if (single) return;  // general
      out = in;
    } else if ((inside = inside_a_sphere(k)) >= 0 && !(want_one && S.sphere_root[size_t(inside)])) {
      return;  // general, all of it
    } else {
      uint32_t tests = 0;
      const uint32_t budget = single ? kTileBudget : kBlockBudget;
      stack.assign(in.rbegin(), in.rend());
      while (!stack.empty()) {
        if (tests >= budget) {
          if (single) return;  // undecided within the budget: general
          out.insert(out.end(), stack.begin(), stack.end());
          break;
        }
        const int32_t n = stack.back();
        stack.pop_back();
        ++tests;
        if (n < 0) {
          if (!prim_touches(k, n)) continue;
          out.push_back(n);
          // a primitive within reach of some ray: general, unless all of them are one sphere
          if (single && !(want_one && sole_sphere(out) >= 0)) return;
          continue;
        }
        const SkyNode& nd = S.nodes[size_t(n)];
        const V c{nd.c[0], nd.c[1], nd.c[2]};
        if (!touches(k, c, nd.r + reach_inner)) continue;
        // a box much smaller than the block's cone is handed down as it is
        if (!single) {
          const V w = c - o;
          if (nd.r + reach_inner < 0.5 * k.s * len(w)) {
            out.push_back(n);
            continue;
          }
        }
        stack.push_back(nd.right);
        stack.push_back(nd.left);
      }
    }
    if (out.empty()) {
      mark(tx0, ty0, tx1, ty1);
      return;
    }
    // what is left is one sphere's primitive alone: a tile is one-sphere; so is a block no
    // tile of which can be sky (every ray runs into that sphere); any other block goes on
    // to its quarters with that one entry (some of them may be sky)
    const int32_t one = want_one ? sole_sphere(out) : -1;
    if (one >= 0) {
      out.resize(1);
      if (single || inside == one) {
        mark(tx0, ty0, tx1, ty1, one);
        return;
      }
    }
    if (single) return;
    const uint32_t mx = tx1 - tx0 > 1 ? tx0 + (tx1 - tx0) / 2 : tx1, my = ty1 - ty0 > 1 ? ty0 + (ty1 - ty0) / 2 : ty1;
    block(tx0, ty0, mx, my, depth + 1);
    if (mx < tx1) block(mx, ty0, tx1, my, depth + 1);
    if (my < ty1) block(tx0, my, mx, ty1, depth + 1);
    if (mx < tx1 && my < ty1) block(mx, my, tx1, ty1, depth + 1);
  }
};
}  // namespace

// ZRT_SKY_TILES=0 turns the split off (default: on).
bool sky_tiles_wanted() {
  const char* e = std::getenv("ZRT_SKY_TILES");
  return !(e && std::atoi(e) == 0);
}
// ZRT_SPHERE_TILES=0 turns the one-sphere class off (default: on; 2: context.cpp).
bool sphere_tiles_wanted() {
  const char* e = std::getenv("ZRT_SPHERE_TILES");
  return !(e && std::atoi(e) == 0);
}

// A launch may split its all-sky tiles off only where the proof above holds and the
// sky kernel computes what the render kernel would: the lockstep FAST loop (general
// or lean kernel), shading (max_depth >= 1), no per-row counters, no guard, the
// camera inside the origin bound (so FAST == reference for its rays).
bool sky_split_allowed(const LaunchPlan& P, const zrt_params* p, bool cam_inside) {
  return P.kmode == 3 && p->max_depth >= 1 && (p->flags & (ZRT_FLAG_SCANLINES | ZRT_FLAG_GUARD)) == 0 && cam_inside;
}
// ... and its one-sphere tiles where, besides, the plan is lean-eligible (plan_launch's
// facts, before the STATS exclusion: the timed and the STATS launch of a frame split
// alike): the one-sphere kernels are instantiated for those two flavours only.
bool sphere_split_allowed(const LaunchPlan& P, const zrt_params* p, bool cam_inside) {
  return sky_split_allowed(P, p, cam_inside) && P.lean;
}

// What the classifier keeps of a flattened scene: per reference-tree node its box's
// bounding sphere, per primitive slot its own, the triangles' reach coefficients.
void build_sky_scene(SkyScene* s, const HostScene& h) {
  *s = SkyScene{};
  if (!h.use_bvh || h.n_nodes == 0 || h.n_nodes > kMaxSkyNodes) return;
  const uint32_t n_slots = uint32_t(h.prims.size() / 3);
  s->prims.resize(n_slots);
  double k_ao = 0.0, k_c = 0.0;
  V tlo{INFINITY, INFINITY, INFINITY}, thi{-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = 0; i < n_slots; ++i) {
    const float4 p0 = h.prims[3 * i], p1 = h.prims[3 * i + 1], p2 = h.prims[3 * i + 2];
    SkyPrim& q = s->prims[i];
    uint32_t tag;
    std::memcpy(&tag, &h.shade[i].w, 4);
    if (!(tag >> 31)) {  // sphere {center.xyz, radius^2}
      const V c{p0.x, p0.y, p0.z};
      const double r = std::sqrt(double(p0.w)) * (1.0 + 0x1p-22);
      if (!finite3(c) || !std::isfinite(r)) return;
      q.c[0] = c.x; q.c[1] = c.y; q.c[2] = c.z;
      q.r = r;
      q.sphere_index = int32_t(s->spheres.size());
      s->spheres.push_back(i);
      continue;
    }
    // triangle {a.xyz, e1.x} {e1.yz, e2.xy} {e2.z, n.xyz}: the f32 edges the tests use
    const V a{p0.x, p0.y, p0.z}, e1{p0.w, p1.x, p1.y}, e2{p1.z, p1.w, p2.x};
    if (!finite3(a) || !finite3(e1) || !finite3(e2)) return;
    const V b = a + e1, c = a + e2, g = (a + b + c) * (1.0 / 3.0);
    q.c[0] = g.x; q.c[1] = g.y; q.c[2] = g.z;
    q.r = std::max({len(a - g), len(b - g), len(c - g)}) * (1.0 + 1e-9);
    q.sphere_index = -1;
    const V n = cross(e1, e2);
    const double nl = len(n);
    // det = -d.n (rounded) stays below the floor 1e-6 whatever the ray: never hit
    if (nl * (1.0 + 1e-4) < 1e-6) {
      q.r = -1.0;
      continue;
    }
    for (const V& v : {a, b, c}) {
      tlo = {std::min(tlo.x, v.x), std::min(tlo.y, v.y), std::min(tlo.z, v.z)};
      thi = {std::max(thi.x, v.x), std::max(thi.y, v.y), std::max(thi.z, v.z)};
    }
    // tools/tri_reach_bound.py: dist(X, T) <= k_ao |ao| + k_c at the reference's det floor
    const double l1 = len(e1), l2 = len(e2), l3 = len(e2 - e1);
    const double smin = std::min({nl / (l1 * l2), nl / (l1 * l3), nl / (l2 * l3)});
    const double cmin = std::min(1e-6 / nl, 1.0);
    k_ao = std::max(k_ao, 8.49 * kU / cmin * (2.0 + (l1 + l2) / l3) / smin);
    k_c = std::max(k_c, (5.83 * kU * l1 * l2 / (cmin * l3) + 3.0 * kU * nl / l3) / smin);
  }
  if (!std::isfinite(k_ao) || !std::isfinite(k_c)) return;
  s->k_ao = 2.0 * k_ao;  // doubled: the bound is first-order
  s->k_c = 2.0 * k_c;
  if (tlo.x <= thi.x) {
    const V c = (tlo + thi) * 0.5;
    s->tri_c[0] = c.x; s->tri_c[1] = c.y; s->tri_c[2] = c.z;
    s->tri_r = len(thi - c) * (1.0 + 1e-9);
    s->has_tri = true;
  }
  s->nodes.resize(h.n_nodes);
  for (uint32_t i = 0; i < h.n_nodes; ++i) {
    const float4 lo = h.nodes[2 * i], hi = h.nodes[2 * i + 1];
    const V a{lo.x, lo.y, lo.z}, b{hi.x, hi.y, hi.z};
    if (!finite3(a) || !finite3(b)) {  // a non-finite plane: no classification
      s->nodes.clear();
      return;
    }
    const V c = (a + b) * 0.5;
    SkyNode& nd = s->nodes[i];
    nd.c[0] = c.x; nd.c[1] = c.y; nd.c[2] = c.z;
    // (a sphere's box is center -+ radius rounded in f32: the slack covers an ulp of each plane)
    nd.r = len(b - c) * (1.0 + 0x1p-20) + 0x1p-20 * (std::fabs(c.x) + std::fabs(c.y) + std::fabs(c.z));
    std::memcpy(&nd.left, &lo.w, 4);
    std::memcpy(&nd.right, &hi.w, 4);
    const auto bad = [&](int32_t ref) {
      return ref >= 0 ? uint32_t(ref) >= h.n_nodes : (uint32_t(-ref - 1) >> 1) >= n_slots;
    };
    if (bad(nd.left) || bad(nd.right)) {
      s->nodes.clear();
      return;
    }
  }
  // the spheres the one-sphere path can stand in for: their reference leaf is a slot of the
  // root wide node (in LDS; every ray's traversal begins there), in the full-node tree
  s->sphere_root.assign(s->spheres.size(), 0);
  s->sphere_args.assign(s->spheres.size(), SphereArgs{});
  if (h.wn.size() >= 8 && h.leaf_of_slot.size() >= n_slots) {
    int32_t ra[4], rb[4];
    std::memcpy(ra, &h.wn[6], 16);
    std::memcpy(rb, &h.wn[7], 16);
    for (size_t i = 0; i < s->spheres.size(); ++i) {
      const uint32_t slot = s->spheres[i], leaf = h.leaf_of_slot[slot];
      if (leaf >= h.n_nodes) continue;
      const int32_t ref = -int32_t(2u * slot) - 1;
      for (int k = 0; k < 4; ++k) {
        if (ra[k] >= 0 || ra[k] == INT32_MIN) continue;  // an inner child, an empty slot
        const int32_t a = ra[k] < -(int32_t(1) << 30) ? ra[k] + (int32_t(1) << 30) : ra[k];
        if (a == ref || rb[k] == ref) s->sphere_root[i] = 1;
      }
      SphereArgs& g = s->sphere_args[i];
      const float4 lo = h.nodes[2 * leaf], hi = h.nodes[2 * leaf + 1], rec = h.prims[3 * slot];
      g.lo[0] = lo.x; g.lo[1] = lo.y; g.lo[2] = lo.z;
      g.hi[0] = hi.x; g.hi[1] = hi.y; g.hi[2] = hi.z;
      g.rec[0] = rec.x; g.rec[1] = rec.y; g.rec[2] = rec.z; g.rec[3] = rec.w;
    }
  }
  s->ok = true;
}

// The class word of each of this rank's tiles (kTileGeneral / kTileSky), their sky count,
// and (m, 4 doubles, optional) the margins: the largest sphere reach, the triangles'
// reach, and its two coefficients.  one (optional, one->want set): the one-sphere tiles
// too (kTileOneSphere | slot), of one sphere only - the one with the most tiles, the
// others' tiles stay general - so that sphere is a constant of the launch.
void classify_tiles(const SkyScene& s, const zrt_camera* cam, const zrt_params* p, std::vector<uint32_t>* cls,
                    uint32_t* n_sky, double* m, OneSphere* one) {
  if (one) {
    one->n_tiles = 0;
    one->sphere = -1;
  }
  const Geometry g = geometry(p);
  const uint32_t mine = rank_tiles(g, p->rank, p->world_size);
  cls->assign(mine, kTileGeneral);
  *n_sky = 0;
  if (m) m[0] = m[1] = m[2] = m[3] = 0.0;
  if (!s.ok || mine == 0) return;
  Classifier C{s};
  C.o = vec(cam->origin);
  C.llc = vec(cam->lower_left_corner);
  C.hor = vec(cam->horizontal);
  C.ver = vec(cam->vertical);
  if (!finite3(C.o) || !finite3(C.llc) || !finite3(C.hor) || !finite3(C.ver)) return;
  C.W = double(float(p->width));
  C.H = double(float(p->height));
  C.xbound = g.xbound;
  C.height = p->height;
  C.tiles_x = g.tiles_x;
  C.tiles_y = g.tiles_y;
  C.rank = p->rank;
  C.world = p->world_size;
  C.cls = cls;
  C.want_one = one && one->want && !s.spheres.empty();
  C.n_one.assign(s.spheres.size(), 0);
  // Camera.getRay in f32: u, v (two roundings and a correctly rounded quotient), two
  // scalings and three sums - each within 2^-24 of a value no larger than the sum S of
  // the four vectors' lengths, so the direction errs by < 2^-21 S (taken: 2^-20 S)
  // against a length of at least the origin's distance h to the image plane; unit()
  // adds a few ulps of angle
  const V nrm = cross(C.hor, C.ver);
  const double nl = len(nrm);
  if (!(nl > 0.0)) return;
  const double h = std::fabs(dot(C.llc - C.o, nrm)) / nl;
  const double S = len(C.llc) + len(C.hor) + len(C.ver) + len(C.o);
  if (!(h > 0.0) || !std::isfinite(S)) return;
  C.eps = 0x1p-20 * S / h + 0x1p-20;
  if (!(C.eps < 1e-2)) return;
  // Spheres (DESIGN.md §3 "Spheres"): the rounded discriminant errs by E <= 32 u (|oc|^2 + r^2),
  // so an accepted ray's line passes within sqrt(r^2 + E) of the centre; E is taken four
  // times (the 2 sqrt(E) of §3, in quadrature with r)
  double reach_sph = 0.0;
  C.sphere_r.resize(s.spheres.size());
  for (size_t i = 0; i < s.spheres.size(); ++i) {
    const SkyPrim& q = s.prims[s.spheres[i]];
    const V oc = C.o - V{q.c[0], q.c[1], q.c[2]};
    const double E = 32.0 * kU * (dot(oc, oc) + q.r * q.r);
    C.sphere_r[i] = std::sqrt(q.r * q.r + 4.0 * E) * (1.0 + 1e-9);
    reach_sph = std::max(reach_sph, C.sphere_r[i] - q.r);
  }
  // Triangles (tools/tri_reach_bound.py, doubled): k_ao |ao| + k_c with |ao| bounded
  // by the camera's distance to the farthest point of the triangles' box
  C.reach_tri = 0.0;
  if (s.has_tri) {
    const double T = len(C.o - V{s.tri_c[0], s.tri_c[1], s.tri_c[2]}) + s.tri_r;
    C.reach_tri = s.k_ao * T + s.k_c;
  }
  C.reach_inner = std::max(reach_sph, C.reach_tri);
  if (!std::isfinite(C.reach_inner)) return;
  // a camera within the triangles' reach of their bounding sphere: no cone can be shown
  // to miss them (the teapot's large triangles, whose first-order reach at the det floor
  // exceeds their distance): every tile is general, at no cost
  if (s.has_tri && !(len(C.o - V{s.tri_c[0], s.tri_c[1], s.tri_c[2]}) > s.tri_r + C.reach_tri)) {
    if (m) {
      m[0] = reach_sph;
      m[1] = C.reach_tri;
      m[2] = s.k_ao;
      m[3] = s.k_c;
    }
    return;
  }
  if (m) {
    m[0] = reach_sph;
    m[1] = C.reach_tri;
    m[2] = s.k_ao;
    m[3] = s.k_c;
  }
  C.frontier.resize(40);
  C.frontier[0].assign(1, 0);  // the reference tree's root
  // a large frame in squares of kSquare x kSquare tiles, dealt to a few threads (each its
  // own classifier state; the squares' tiles are disjoint): C4's 65 536 tiles take 7 ms on one
  constexpr uint32_t kSquare = 32;
  const uint32_t sq_x = (g.tiles_x + kSquare - 1) / kSquare, sq_y = (g.tiles_y + kSquare - 1) / kSquare;
  const uint32_t n_strips = sq_x * sq_y;
  const uint32_t n_thr = std::min({8u, std::max(1u, std::thread::hardware_concurrency()), n_strips / 4u});
  // the one-sphere tiles of every sphere but the one with the most (the lowest index among equals) go back to general
  const auto keep_one = [&](const std::vector<uint32_t>& n_one) {
    if (!C.want_one) return;
    size_t best = 0;
    for (size_t i = 1; i < n_one.size(); ++i)
      if (n_one[i] > n_one[best]) best = i;
    if (n_one[best] == 0) return;
    const uint32_t word = kTileOneSphere | s.spheres[best];
    for (uint32_t& w : *cls)
      if ((w & kTileOneSphere) && !(w & kTileSky) && w != word) w = kTileGeneral;
    one->n_tiles = n_one[best];
    one->sphere = int32_t(best);
  };
  if (n_thr <= 1) {
    C.block(0, 0, g.tiles_x, g.tiles_y, 0);
    *n_sky = C.n_sky;
    keep_one(C.n_one);
    return;
  }
  std::atomic<uint32_t> next{0}, total{0};
  std::vector<std::atomic<uint32_t>> total_one(s.spheres.size());
  for (auto& t : total_one) t.store(0);
  const auto work = [&]() {
    Classifier W = C;
    for (uint32_t i = next.fetch_add(1); i < n_strips; i = next.fetch_add(1))
      W.block((i % sq_x) * kSquare, (i / sq_x) * kSquare, std::min(g.tiles_x, (i % sq_x + 1) * kSquare),
              std::min(g.tiles_y, (i / sq_x + 1) * kSquare), 0);
    total.fetch_add(W.n_sky);
    for (size_t i = 0; i < W.n_one.size(); ++i) total_one[i].fetch_add(W.n_one[i]);
  };
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < n_thr; ++t) pool.emplace_back(work);
  work();
  for (std::thread& t : pool) t.join();
  *n_sky = total.load();
  std::vector<uint32_t> n_one(total_one.size());
  for (size_t i = 0; i < n_one.size(); ++i) n_one[i] = total_one[i].load();
  keep_one(n_one);
}
}  // namespace zrt
