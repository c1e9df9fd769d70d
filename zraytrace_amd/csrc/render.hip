// render.hip — the MI355X path of the reference's per-pixel sampling loop.
//
// Replaces raytrace.render (raytrace.zig:136-203) + rayColor (:62-100) and
// everything they call per sample: Camera.getRay (camera.zig:46-52), BVH/AABB
// traversal (bvh.zig:187-205, aabb.zig:109-127), Sphere.hit / Triangle.hit
// (sphere.zig:31-71, triangle.zig:48-70), HitRecord.init (hit_record.zig:28-41),
// Material.scatter (material.zig:43-129), Sample.randomUnitVector
// (sample.zig:47-61), Texture.albedo (texture.zig:20-74).
//
// Kernel structure (gfx950, wave64):
//   * persistent grid (CUs x resident blocks), 256-thread blocks;
//   * each lane owns one pixel at a time and walks its samples in order, so
//     the per-pixel f32 sum is accumulated exactly as raytrace.zig:172-179
//     does; when a lane's path ends it immediately starts the next sample, and
//     when its pixel is done the wave refills its finished lanes from a global
//     work counter with ONE atomic per wave (__ballot + popcount + mbcnt rank);
//   * the recursion `attenuation * rayColor(...)` is unrolled into an
//     iterative loop; the attenuations are stacked per lane and multiplied in
//     reverse at path end so the product keeps the recursion's association;
//   * BVH traversal uses a per-lane stack in LDS laid out [depth][lane]
//     (conflict-free: every lane of a wave hits a distinct bank);
//   * RNG: one Xoroshiro128+ (or Xoshiro256++) stream per (pixel, sample),
//     seeded through SplitMix64 exactly as DefaultPrng.init seeds.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <type_traits>

#include "accel_build.hpp"
#include "device_math.hpp"
#include "kernels.hpp"
#include "zrt.hpp"

namespace zrt {

// The STATS flavour's bounds check of a global row index (attenuation rows,
// stack overflow rows) against its buffer (KArgs::att_cap / ovf_cap, set from the
// allocations): past it, kErrBounds is raised and the access skipped, so a
// sizing mistake the host check (zrt::check_buffers) missed reports instead of
// faulting.  The timed flavour compiles it away.
template <bool STATS>
__device__ __forceinline__ bool row_ok(const KArgs& a, uint64_t idx, uint64_t cap) {
  if (!STATS || idx < cap) return true;
  atomicOr(a.error_flag, kErrBounds);
  return false;
}

// Kernel arguments that only rare branches of the FAST loop read (the error flag, the
// stack's overflow rows, the replay's reference tree) are loaded from the argument
// block inside those branches, through a pointer the compiler cannot trace: they do
// not sit in (spilled) SGPRs across the sampling loop.
// The kernel's arguments as a rare branch reads them.  Every kernel that reaches these
// paths takes its KArgs by value as its first parameter, so the argument block starts
// with it; the empty asm hides where the pointer came from, which keeps each load - a
// scalar load from the constant address space - inside the branch that asked for it.
// (The host pass only needs the code to compile.)
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) KArgs* RareArgs;
__device__ __forceinline__ RareArgs rare_args(const KArgs& a) {
  (void)a;
  RareArgs p = (RareArgs)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(p));
  return p;
}
#else
typedef const KArgs* RareArgs;
__device__ __forceinline__ RareArgs rare_args(const KArgs& a) { return &a; }
#endif
// the device error flag raised (stack overflow, a tree the kernel does not decode, ...)
__device__ __forceinline__ void raise_error(const KArgs& a, uint32_t bits) { atomicOr(rare_args(a)->error_flag, bits); }
// lane gl's column of the FAST stack's rows past the LDS part ([row][lane] in global memory)
template <class StackT>
__device__ __forceinline__ StackT* ovf_column(const KArgs& a, uint32_t gl) {
  return reinterpret_cast<StackT*>(rare_args(a)->stack_ovf) + gl;
}

// ZRT_PROFILE builds (diagnostic only, never the shipped library) add s_memtime
// cycle sums per loop section into counters[kProfSlot + section].
#ifndef ZRT_PROFILE
#define ZRT_PROFILE 0
#endif
__device__ __forceinline__ uint64_t prof_stamp() {
  uint64_t t = 0;
#if ZRT_PROFILE
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
#endif
  return t;
}

#ifndef ZRT_PROBE_SPP
#define ZRT_PROBE_SPP 1  // samples per pixel of the scheduling probe; A/B at N=8: 1, 2, 4, 8 give the same render launch
#endif
#ifndef ZRT_STACK_ROWS_LOCK
#define ZRT_STACK_ROWS_LOCK 16  // lockstep FAST loop: traversal stack rows in LDS (deeper rows in global memory)
#endif
#ifndef ZRT_SYNC_SAMPLES
#define ZRT_SYNC_SAMPLES 1  // the lanes of a wave wait for each other every this many samples
#endif
// The lean lockstep kernel (render_kernel<3, PRNG, false, StackT, true>, DESIGN.md §3
// "The lean kernel"): the timed FAST lockstep loop compiled for a scene of
// solid-colour Lambertian and metal materials only, whose triangles all pass the
// tri_rcp_fast bound, rendered from a camera inside the origin bound, without
// scanline rows (zrt::plan_launch's `lean` and the launch's own check_origins
// decide on the host; ZRT_LEAN=0 forces the general kernel).  The features it
// leaves out:
//   tex     no image textures: no (u, v), no texel codes, no texel stores in att_value
//   diel    no dielectric: no refraction branch, no (1, 1, 1) attenuation code
//   origin  every ray origin inside the bound: ray_origin_ok is true
//   epi     no scanline rows and no probe cost at the end of a unit
// (It keeps the IEEE 1/det behind dev::rcp_core: dropping that alone spilt 30 VGPRs
// for 26, and the other four without it ran C4 0.4 % faster than all five.)
template <bool LEAN>
struct Lean {
  static constexpr bool tex = LEAN, diel = LEAN, origin = LEAN, epi = LEAN;
};

// ---------------------------------------------------------------------------
// RNG: std.rand DefaultPrng restated per (pixel, sample)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }
__device__ __forceinline__ uint64_t splitmix_next(uint64_t& s) {
  s += 0x9e3779b97f4a7c15ULL;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}

template <int PRNG>
struct Rng;

template <>
struct Rng<ZRT_PRNG_XOROSHIRO128> {
  uint64_t s0, s1;
  __device__ __forceinline__ void init(uint64_t key) {
    uint64_t g = key;
    s0 = splitmix_next(g);
    s1 = splitmix_next(g);
  }
  __device__ __forceinline__ uint64_t next() {  // Xoroshiro128+
    const uint64_t a = s0;
    uint64_t b = s1;
    const uint64_t r = a + b;
    b ^= a;
    s0 = rotl64(a, 55) ^ b ^ (b << 14);
    s1 = rotl64(b, 36);
    return r;
  }
};

template <>
struct Rng<ZRT_PRNG_XOSHIRO256> {
  uint64_t s[4];
  __device__ __forceinline__ void init(uint64_t key) {
    uint64_t g = key;
    s[0] = splitmix_next(g);
    s[1] = splitmix_next(g);
    s[2] = splitmix_next(g);
    s[3] = splitmix_next(g);
  }
  __device__ __forceinline__ uint64_t next() {  // Xoshiro256++
    const uint64_t r = rotl64(s[0] + s[3], 23) + s[0];
    const uint64_t t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl64(s[3], 45);
    return r;
  }
};

// Random.float(f32) / Random.boolean()
template <class R>
__device__ __forceinline__ float rand_float(R& r) {
  const uint32_t s = (uint32_t)r.next();
  return __uint_as_float((0x7fu << 23) | (s >> 9)) - 1.0f;
}
template <class R>
__device__ __forceinline__ bool rand_bool(R& r) {
  return (r.next() & 1u) != 0;
}
// r = c ? t : r, word by word (a lane keeps the state it advanced only where it drew)
template <class R>
__device__ __forceinline__ void rng_keep(R& r, const R& t, bool c) {
  uint32_t a[sizeof(R) / 4], b[sizeof(R) / 4];
  __builtin_memcpy(a, &r, sizeof(a));
  __builtin_memcpy(b, &t, sizeof(b));
#pragma unroll
  for (uint32_t k = 0; k < sizeof(R) / 4; ++k) a[k] = c ? b[k] : a[k];
  __builtin_memcpy(&r, a, sizeof(a));
}

// ---------------------------------------------------------------------------
// small vector helpers (evaluation order as vector.zig)
// ---------------------------------------------------------------------------
struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 mk(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 u, V3 v) {
  return mk(u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x);
}
__device__ __forceinline__ V3 add(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 scale(V3 a, float s) { return mk(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ V3 neg(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ V3 unit(V3 v) {  // vector.zig:88-92
  const float l = dev::sqrt_rn(v.x * v.x + v.y * v.y + v.z * v.z);
  // v.k / l as dev::div_core over one reciprocal of l (12 VALU instead of 30):
  // bit-identical to the three IEEE divisions while l lies in [2^-50, 2^50] and
  // every quotient in [2^-51, 1]; a zero / tiny component or a degenerate l takes
  // the IEEE divisions (zero's sign, NaN of 0/0, inf)
  // (the range is checked on the operands, |v.k| >= l * 2^-50, before any quotient
  // exists, so each component's three steps need two registers at a time)
  const float vmin = __builtin_fminf(__builtin_fminf(__builtin_fabsf(v.x), __builtin_fabsf(v.y)), __builtin_fabsf(v.z));
  if (__builtin_expect(ZRT_FAST_DIV && l >= 0x1p-50f && l <= 0x1p50f && vmin >= l * 0x1p-50f, 1)) {
    const float y = dev::rcp_core(l);
    return mk(dev::div_core(v.x, l, y), dev::div_core(v.y, l, y), dev::div_core(v.z, l, y));
  }
  return mk(v.x / l, v.y / l, v.z / l);
}
// 1/d of aabb.zig:112 (one IEEE division per axis), bit for bit: dev::rcp_core
// while every |d.k| lies in [2^-126, 2^126), else the IEEE divisions
__device__ __forceinline__ void inv_dir(float dx, float dy, float dz, float& ix, float& iy, float& iz) {
  const float lo = __builtin_fminf(__builtin_fminf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz));
  const float hi = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(dx), __builtin_fabsf(dy)), __builtin_fabsf(dz));
  if (__builtin_expect(ZRT_FAST_DIV && lo >= 0x1p-126f && hi < 0x1p126f, 1)) {
    ix = dev::rcp_core(dx);
    iy = dev::rcp_core(dy);
    iz = dev::rcp_core(dz);
  } else {
    ix = 1.0f / dx;
    iy = 1.0f / dy;
    iz = 1.0f / dz;
  }
}
// 1/det of triangle.zig:63 for det >= 1e-6 (the only dets the hit test uses).
// `fast` (wave-uniform, RayT::rcp_det): the scene's triangles keep det below
// 2^126, so dev::rcp_core needs no per-lane guard (a per-lane branch here, in the
// leaf loop, cost the FAST kernel 4 spilled VGPRs)
__device__ __forceinline__ float inv_det_rn(float det, uint32_t fast) {
  if (ZRT_FAST_DIV && fast) return dev::rcp_core(det);
  return 1.0f / det;
}
__device__ __forceinline__ V3 reflect(V3 v, V3 n) { return sub(v, scale(n, 2.0f * dot(v, n))); }
__device__ __forceinline__ V3 refract(V3 v, V3 n, float ratio) {  // vector.zig:132-137
  const float cos_theta = dev::fmin_z(dot(neg(v), n), 1.0f);
  const V3 perp = scale(add(v, scale(n, cos_theta)), ratio);
  const V3 par = scale(n, -dev::sqrt_rn(__builtin_fabsf(1.0f - (perp.x * perp.x + perp.y * perp.y + perp.z * perp.z))));
  return add(perp, par);
}

// ---------------------------------------------------------------------------
// traversal
// ---------------------------------------------------------------------------
struct RayT {
  float ox, oy, oz;
  float ix, iy, iz;  // 1/d per axis (aabb.zig:112 computes it per test; same bits)
  float dx, dy, dz;
  // 1 when every triangle of the scene has |n| < 2^125 (host check), so a det of
  // triangle.zig:61 that passes det >= 1e-6 lies in dev::rcp_core's range; a
  // wave-uniform value (from KArgs), so the choice below is a scalar branch
  uint32_t rcp_det;
  // the scene's grazing-margin coefficient (KArgs::graze_m, 2^-18 by default);
  // wave-uniform, so it stays in SGPRs
  float gm;
  // KArgs::graze_leaf.  Nothing reads it (leaf slots share gm); it stays, filled, until
  // KArgs::graze_leaf goes: without it the register allocation of every kernel changes
  float gl;
  float gk;  // the grazing-triangle guard's coefficient (KArgs::guard; 0: off), wave-uniform
};

// A computed primitive hit lies outside its own box: a triangle's by a few ulps
// of the coordinates involved, about 2^-23 x (t + the triangle's largest
// |coordinate|) (|o| <= t + that, so the origin adds nothing); a sphere's only
// along the ray (its point is o + t d), i.e. by its error in t.  In t that is
// the distance times |1/d_k| on the axis it is measured along, unbounded for a
// ray (nearly) parallel to a box face: the relative margin alone culled boxes the
// reference opens and hits in (DESIGN.md §3 "Grazing rays").  So:
// * the t-proportional part: every narrowed cull's relative margin is
//   1 + 2^-16 + 2^-18 max_k |1/d_k| (ray_rel, per ray);
// * the coordinate part, inner wide slots: their boxes are stored grown by
//   2^-19 x their own largest |coordinate| (accel_build.cpp), which grows each
//   axis's t interval by exactly that distance x |1/d_k|, at no cost per node;
// * the coordinate part, reference boxes (leaf slots, the BINARY traversal, the
//   replay), which stay bit for bit: a uniform slack 2^-18 x the triangles'
//   largest |coordinate| x max_k |1/d_k| (ray_slack).  A leaf slot failing the
//   narrowed test by less is decided by loose_slot: the reference's own
//   per-axis test, and the narrowed test of the leaf's box grown by its own
//   coordinates.
// On the grazing rays no hit lies outside its box's t interval by more than 0.72
// of half these margins (tools/grazing_excess.py).
// (recomputed where used from 1/d, 1 VALU each, rather than kept in VGPRs across
// the traversal: two more live registers cost the deep-tree loop spills)
__device__ __forceinline__ float ray_m(const RayT& r) {  // max_k |1/d_k|
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(r.ix), __builtin_fabsf(r.iy)), __builtin_fabsf(r.iz));
}
// relative margin of every narrowed cull: 1 + 2^-16 + 2^-18 m
__device__ __forceinline__ float ray_rel(const RayT& r, float m) { return 1.0000153f + r.gm * m; }
// the reference boxes' slack: 2^-18 x the triangles' largest |coordinate| x m
__device__ __forceinline__ float ray_slack(const RayT& r, float extent, float m) {
  return __builtin_fmaxf(extent, 0x1p-100f) * r.gm * m;
}

// Nearly axis-parallel rays (DESIGN.md §3 "Per-axis margins").  The margins
// above are t-space terms scaled by m = max_k |1/d_k| on every axis, but a hit's
// excess beyond its box is a distance in space: e (t + coordinates), on axis k
// e (t + coordinates) |1/d_k| in t.  Only an axis the ray runs (nearly) parallel
// to needs the large term; applied to all three it turns the narrowed cull off
// (m = 2^20: every exit x 5) and such a ray walks most of the tree.  A wave with
// a lane whose m exceeds kPaxisM (a wave-uniform branch) therefore widens each
// axis of every slot by its own term g |1/d_k|, g = 2^-18 (T + extent) (T: the
// ray's farthest distance to the triangles' box, which bounds the hit's t; extent:
// the triangles' largest |coordinate|, ray_slack's spatial term) - 6 more adds
// per slot, for waves with such a lane only; the other waves keep ray_rel with
// m <= kPaxisM.
// (The lockstep loop keeps the t-space margins: its 96-VGPR budget spills 7 -> 28
// registers with the branch, C4 -2.8 %.  A leaf-only margin from a coefficient of
// its own, KArgs::graze_leaf, fixed none of the grazing-triangle misses at C4 -4 %,
// profiles/r04/r04c: leaf slots share ray_rel.)
#ifndef ZRT_PAXIS_LOG2M
#define ZRT_PAXIS_LOG2M 10
#endif
constexpr float kPaxisM = float(1u << ZRT_PAXIS_LOG2M);
__device__ __forceinline__ float paxis_grow(const KArgs& a, const RayT& r) {
  const float T = (__builtin_fabsf(r.ox - a.tri_c[0]) + a.tri_h[0]) + (__builtin_fabsf(r.oy - a.tri_c[1]) + a.tri_h[1]) +
                  (__builtin_fabsf(r.oz - a.tri_c[2]) + a.tri_h[2]);  // >= the L2 distance to any corner
  return (T + __builtin_fmaxf(a.scene_extent, 0x1p-100f)) * (r.gm * 1.0000153f);  // (rounding of T: the extra 2^-16)
}
// the per-axis term in t, finite (an infinite 1/d_k keeps the slab's exact +-inf:
// the reference's own test then rejects every leaf off the plane)
__device__ __forceinline__ float paxis_t(float g, float inv) {
  return __builtin_fminf(g * __builtin_fabsf(inv), 0x1p126f);
}
// The grazing-triangle guard's spatial widening for this ray: gk (T + extent)
// (T as in paxis_grow bounds |o - a| for every triangle vertex a): the reach of
// an accepted hit beyond its triangle, k |ao| + k_c (DESIGN.md §3 "Triangles").
__device__ __forceinline__ float guard_grow(const KArgs& a, const RayT& r) {
  const float T = (__builtin_fabsf(r.ox - a.tri_c[0]) + a.tri_h[0]) + (__builtin_fabsf(r.oy - a.tri_c[1]) + a.tri_h[1]) +
                  (__builtin_fabsf(r.oz - a.tri_c[2]) + a.tri_h[2]);
  return (T + __builtin_fmaxf(a.scene_extent, 0x1p-100f)) * (r.gk * 1.0000153f);
}

// aabb.zig:109-127: each axis against [t_min, t_max] on its own.
// FAST additionally narrows the interval across axes (with a 2^-16 relative
// margin) and reports the entry distance for near-first ordering.
// gw: the grazing-triangle guard's spatial widening of the narrowed test (per
// axis gw |1/d_k|; 0: none) - the loose test stays the reference's own
template <bool FAST>
__device__ __forceinline__ bool box_test(const float4 lo, const float4 hi, const RayT& r, float t_max,
                                         float* entry, float slack = 0.0f, bool narrow = true, float gw = 0.0f) {
  const float t_min = 0.001f;
  float a0 = (lo.x - r.ox) * r.ix, a1 = (hi.x - r.ox) * r.ix;
  float b0 = (lo.y - r.oy) * r.iy, b1 = (hi.y - r.oy) * r.iy;
  float c0 = (lo.z - r.oz) * r.iz, c1 = (hi.z - r.oz) * r.iz;
  if (r.ix < 0.0f) { const float t = a0; a0 = a1; a1 = t; }
  if (r.iy < 0.0f) { const float t = b0; b0 = b1; b1 = t; }
  if (r.iz < 0.0f) { const float t = c0; c0 = c1; c1 = t; }
  // math.max(t0, t_min) / math.min(t1, t_max) are `x > y ? x : y` / `x < y ? x : y`.
  // With a non-NaN second operand (t_min, t_max never are) these equal IEEE
  // maxNum / minNum (v_max_f32 / v_min_f32) for every NaN first operand, and
  // differ only in the sign of a zero result, which no comparison below sees.
  const float an = __builtin_fmaxf(a0, t_min), ax = __builtin_fminf(a1, t_max);
  const float bn = __builtin_fmaxf(b0, t_min), bx = __builtin_fminf(b1, t_max);
  const float cn = __builtin_fmaxf(c0, t_min), cx = __builtin_fminf(c1, t_max);
  bool ok = (ax > an) && (bx > bn) && (cx > cn);  // !(tmax <= tmin) for every axis
  if (FAST) {
    const float en = __builtin_fmaxf(__builtin_fmaxf(an, bn), cn);
    const float ex = __builtin_fminf(__builtin_fminf(ax, bx), cx);
    if (__builtin_expect(gw > 0.0f, 0)) {  // (a scalar branch: gw is the scene's guard)
      const float wa = paxis_t(gw, r.ix), wb = paxis_t(gw, r.iy), wc = paxis_t(gw, r.iz);
      const float enw = __builtin_fmaxf(__builtin_fmaxf(a0 - wa, b0 - wb), __builtin_fmaxf(c0 - wc, t_min));
      const float exw = __builtin_fminf(__builtin_fminf(a1 + wa, b1 + wb), __builtin_fminf(c1 + wc, t_max));
      ok = ok && (!narrow || !(enw > __builtin_fmaf(exw, ray_rel(r, ray_m(r)), slack)));
    } else {
      ok = ok && (!narrow || !(en > __builtin_fmaf(ex, ray_rel(r, ray_m(r)), slack)));
    }
    *entry = en;
  }
  return ok;
}

__device__ __forceinline__ int as_int(float f) { return __float_as_int(f); }

// Order hazards.  The reference tests each leaf against the best
// hit of the leaves before it in its DFS order, so the hit FAST finds closest is
// one the reference never reaches when a hit of another leaf lies between it and
// its own leaf's loose entry (the two roundings disagree at shared vertices on a
// box face).  TRACK flags such near ties in the sign bit of best_t (a hit's t is
// > t_min > 0; every reader takes |best_t|, a free source modifier), so the
// flag costs no register: set when another hit lies within kNearTie of the best.
constexpr float kNearTie = 1.00006104f;  // 1 + 2^-14
// FAST opens every box whose entry lies below best * kOpen: 1 + 2^-12 (exact in
// f32).  With the near-tie band f = 2^-14 this is exact for any scene whose
// primitive hits lie in their leaf's box up to a relative m < 2^-12 - 2^-14
// ("Exactness"; the REFERENCE traversal's STATS flavour
// measures m: zrt_stats.box_excess_max_*).  Round 1 used 1 + 2^-16 here, which
// left the verdict's band (1 + 2^-15, 1 + 2^-14] unguarded.
constexpr float kOpen = 1.000244140625f;

template <bool TIE, bool TRACK>
__device__ __forceinline__ void accept_hit(float t, int slot, float& best_t, int& best, const RayT& r,
                                           float entry) {
  if (!TRACK) {
    const bool in_range = TIE ? (t < best_t || (t == best_t && slot < best)) : (t < best_t);
    if (in_range) {
      best_t = t;
      best = slot;
    }
    return;
  }
  const float bt = __builtin_fabsf(best_t);
  if (t < bt || (t == bt && slot < best)) {
    bool near = t < bt ? bt <= t * kNearTie : best_t < 0.0f;  // an equal-t swap keeps the flag
    // FAST: the leaf's loose entry E (aabb.zig:109-127, >= t_min > 0; the slot's
    // `en` of wide_iter, bit for bit) above the hit by more than the band also
    // flags the ray; entry < 0: no leaf entry to check (the other traversals)
    near = near || entry > t * kNearTie;
    best_t = near ? -t : t;
    best = slot;
  } else if (t > bt && t <= bt * kNearTie) {
    best_t = -bt;
  }
}

// Triangle.hit (triangle.zig:48-70) for the candidate slot; accepts when the
// reference would (det >= 1e-6, t_min < t < t_max, u,v >= 0, u+v <= 1), with
// equal-t ties going to the lower slot (= earlier in the reference's DFS).
template <bool TIE, bool TRACK = false>
__device__ __forceinline__ void tri_test_v(const float4 p0, const float4 p1, const float4 p2, int slot,
                                           const RayT& r, float& best_t, int& best, float entry = -1.0f) {
  const V3 n = mk(p2.y, p2.z, p2.w);
  const V3 d = mk(r.dx, r.dy, r.dz);
  const float det = -dot(d, n);
  if (!(det >= 1e-6f)) return;
  const float inv_det = inv_det_rn(det, r.rcp_det);
  const V3 ao = mk(r.ox - p0.x, r.oy - p0.y, r.oz - p0.z);
  const V3 dao = cross(ao, d);
  const V3 e1 = mk(p0.w, p1.x, p1.y);
  const V3 e2 = mk(p1.z, p1.w, p2.x);
  const float u = dot(e2, dao) * inv_det;
  const float v = -dot(e1, dao) * inv_det;
  const float t = dot(ao, n) * inv_det;
  if (t > 0.001f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f) accept_hit<TIE, TRACK>(t, slot, best_t, best, r, entry);
}

template <bool TIE, bool TRACK = false>
__device__ __forceinline__ void tri_test(const float4* __restrict__ prims, int slot, const RayT& r,
                                         float& best_t, int& best, float entry = -1.0f) {
  tri_test_v<TIE, TRACK>(prims[3 * slot + 0], prims[3 * slot + 1], prims[3 * slot + 2], slot, r, best_t, best,
                         entry);
}

// Sphere.hit (sphere.zig:31-41, 53-56): nearest root in (t_min, t_max).
template <bool TIE, bool TRACK = false>
__device__ __forceinline__ void sphere_test(const float4 c, int slot, const RayT& r, float& best_t,
                                            int& best, float entry = -1.0f) {
  const V3 oc = mk(r.ox - c.x, r.oy - c.y, r.oz - c.z);
  const V3 d = mk(r.dx, r.dy, r.dz);
  const float half_b = dot(oc, d);
  const float cc = (oc.x * oc.x + oc.y * oc.y + oc.z * oc.z) - c.w;  // c.w = RN(r * r)
  const float disc = half_b * half_b - cc;
  if (disc < 0.0f) return;
  const float root = dev::sqrt_rn(disc);
  const float t1 = -half_b - root;
  const float t = (t1 > 0.001f) ? t1 : (-half_b + root);
  if (t > 0.001f) accept_hit<TIE, TRACK>(t, slot, best_t, best, r, entry);
}

template <bool TIE, bool STATS, bool TRACK = false>
__device__ __forceinline__ void prim_test(const float4* __restrict__ prims, int ref, const RayT& r,
                                          float& best_t, int& best, uint32_t& c_tri, uint32_t& c_sph,
                                          float entry = -1.0f) {
  const int code = -ref - 1;
  const int slot = code >> 1;
  if (code & 1) {
    if (STATS) ++c_tri;
    tri_test<TIE, TRACK>(prims, slot, r, best_t, best, entry);
  } else {
    if (STATS) ++c_sph;
    sphere_test<TIE, TRACK>(prims[3 * slot], slot, r, best_t, best, entry);
  }
}

// prim_test for a WAVE-UNIFORM ref: the record is read with scalar loads
// (s_load through the constant address space), so the 48 bytes do not cross
// the vector data return (TD), which is what the FAST loop saturates (DESIGN.md
// §4); on the bunny 89 % of the leaf trips test one primitive in every active
// lane (tools/simd_eff.py uniform_prim_frac).  Same arithmetic as prim_test.
template <bool TIE, bool STATS, bool TRACK = false>
__device__ __forceinline__ void prim_test_uniform(const float4* __restrict__ prims, int ref, const RayT& r,
                                                  float& best_t, int& best, uint32_t& c_tri, uint32_t& c_sph,
                                                  float entry = -1.0f) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) float4 cfloat4;
  cfloat4* cp = (cfloat4*)prims;
#else
  const float4* cp = prims;
#endif
  const int code = -ref - 1;
  const int slot = code >> 1;
  if (code & 1) {
    if (STATS) ++c_tri;
    tri_test_v<TIE, TRACK>(cp[3 * slot + 0], cp[3 * slot + 1], cp[3 * slot + 2], slot, r, best_t, best, entry);
  } else {
    if (STATS) ++c_sph;
    sphere_test<TIE, TRACK>(cp[3 * slot], slot, r, best_t, best, entry);
  }
}

// The reference's loose entry of a box (aabb.zig:109-127): the largest per-axis
// max(t0, t_min) after the swap of aabb.zig:116-118, the t_max a test of the box
// needs to exceed.
__device__ __forceinline__ float loose_entry(const float4 lo, const float4 hi, const RayT& r) {
  const float nx = ((r.ix < 0.0f ? hi.x : lo.x) - r.ox) * r.ix;
  const float ny = ((r.iy < 0.0f ? hi.y : lo.y) - r.oy) * r.iy;
  const float nz = ((r.iz < 0.0f ? hi.z : lo.z) - r.oz) * r.iz;
  return __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, 0.001f));
}

// Order hazard of a hit found by a near-first traversal (best_t's sign cleared
// here): a near tie was flagged (the reference may reach the other hit first and
// then reject the best's leaf), or the loose entry E of the best's own reference
// leaf lies above the best hit by more than the near-tie band (hits in leaves
// culled against the best could then be below E).  Such rays are traced again
// the reference's way.
template <bool ENTRY>
__device__ __forceinline__ bool order_hazard(const KArgs& a, const RayT& r, float& best_t, int best) {
  const bool near = best_t < 0.0f;
  best_t = __builtin_fabsf(best_t);
  if (best < 0) return false;
  if (near || !ENTRY) return near;  // FAST folds the entry test into the flag (accept_hit)
  const uint32_t leaf = a.leaf_of_slot[best];  // the reference BVH node holding slot `best`
  const float e = loose_entry(a.nodes[2 * leaf], a.nodes[2 * leaf + 1], r);
  return e > best_t * kNearTie;
}

// The geometry of a primitive hit alone (t_max = inf): its t, or +inf.  Used by
// the REFERENCE traversal's STATS flavour to measure how far the hits the
// reference computes lie outside their own leaf's box (box_excess_*).
__device__ __forceinline__ float prim_hit_t(const float4* __restrict__ prims, int ref, const RayT& r) {
  const int code = -ref - 1;
  const int slot = code >> 1;
  float t = __builtin_inff();
  int b = -1;
  if (code & 1) tri_test<false>(prims, slot, r, t, b);
  else sphere_test<false>(prims[3 * slot], slot, r, t, b);
  return t;
}

// max(E / t - 1, t / X - 1) for a hit t in a leaf whose loose entry is E and
// whose exit (min over axes of the far slab distance) is X: > 0 when the
// rounded hit lies before the box's entry or past its exit.
__device__ __forceinline__ float box_excess(const float4 lo, const float4 hi, const RayT& r, float t) {
  const float e = loose_entry(lo, hi, r);
  const float xx = ((r.ix < 0.0f ? lo.x : hi.x) - r.ox) * r.ix;
  const float xy = ((r.iy < 0.0f ? lo.y : hi.y) - r.oy) * r.iy;
  const float xz = ((r.iz < 0.0f ? lo.z : hi.z) - r.oz) * r.iz;
  const float x = __builtin_fminf(__builtin_fminf(xx, xy), xz);
  return __builtin_fmaxf(e / t - 1.0f, t / x - 1.0f);
}

struct ExcessAcc {
  float tri = 0.0f, sph = 0.0f;
  uint32_t over = 0;  // hits outside their box by more than 2^-14
  __device__ __forceinline__ void leaf(const float4* __restrict__ prims, const float4 lo, const float4 hi,
                                       const RayT& r, int ra, int rb) {
    for (int k = 0; k < 2; ++k) {
      const int ref = k == 0 ? ra : rb;
      if (k == 1 && rb == ra) break;
      const float t = prim_hit_t(prims, ref, r);
      if (t == __builtin_inff()) continue;
      const float ex = box_excess(lo, hi, r, t);
      if (!(ex > 0.0f)) continue;
      if ((-ref - 1) & 1) tri = __builtin_fmaxf(tri, ex);
      else sph = __builtin_fmaxf(sph, ex);
      over += ex > 6.1035156e-05f ? 1u : 0u;
    }
  }
};

// A ray whose origin lies where the wide tree's sphere growth was sized for
// (KArgs::origin_bound, DESIGN.md §3 "Spheres"); other rays (none in a render of
// the reference's scenes: their cameras lie inside that region) are traced the
// reference's way alone.
__device__ __forceinline__ bool ray_origin_ok(const KArgs& a, const RayT& r) {
  if (!a.check_origins) return true;  // (wave-uniform: a scalar branch)
  const float m = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(r.ox - a.root_c[0]), __builtin_fabsf(r.oy - a.root_c[1])),
                                  __builtin_fabsf(r.oz - a.root_c[2]));
  return m <= a.origin_bound;
}

// The reference's traversal (bvh.zig:187-205) for a ray FAST flagged: left-first
// over the reference BVH, every box through the reference's loose test against the
// current best, so every leaf is accepted or rejected as the reference does.
// narrow: also cull boxes the ray does not cross (the narrowed test with the
// grazing slack) - except boxes holding a sphere, whose rounded
// test reaches beyond the sphere (KArgs::ref_sph); false: the reference's test alone.
template <class StackT>
__device__ __forceinline__ void reference_replay(const KArgs& a, const RayT& ray, StackT* __restrict__ stk, uint32_t gl,
                                                 float& best_t, int& best, bool narrow = true) {
#if defined(__HIP_DEVICE_COMPILE__)
  // box_test swaps each axis' planes by the sign of 1/d: the same comparisons as the
  // octant's (wide_view), which the compiler would make once per ray and keep - spilled
  // to six lanes per ray - for this branch almost no ray takes.  The copies below hold
  // the same values, but their comparisons are made here.
  RayT r = ray;
  asm volatile("" : "+v"(r.ix), "+v"(r.iy), "+v"(r.iz));
#else
  const RayT& r = ray;
#endif
  // (the reference tree, its stack depth and the overflow rows are read here only)
  const RareArgs ra = rare_args(a);
  const uint32_t rows = a.lds_rows, cap = ra->ref_stack;
  StackT* __restrict__ ovf = reinterpret_cast<StackT*>(ra->stack_ovf) + gl;
  const float4* __restrict__ nodes = ra->nodes;
  const uint8_t* __restrict__ ref_sph = ra->ref_sph;
  const float slack = ray_slack(r, a.scene_extent, ray_m(r));
  const float gw = r.gk > 0.0f ?guard_grow(a, r) : 0.0f;  // the grazing-triangle guard
  best_t = __builtin_inff();
  best = -1;
  uint32_t c_tri = 0, c_sph = 0;
  stk[0] = 0;
  uint32_t sp = 1;
  while (sp > 0) {
    --sp;
    const int idx = sp < rows ? (int)stk[sp * kBlock] : (int)ovf[(size_t)(sp - rows) * a.n_lanes];
    const float4 lo = nodes[2 * idx], hi = nodes[2 * idx + 1];
    float e;
    // the reference's loose test against the current best, and FAST's narrowed
    // emptiness test (a box the ray does not cross holds no hit):
    // left-first with the reference's t_max, so every leaf is accepted or
    // rejected exactly as the reference does it, in ~1 % of its node visits
    if (!box_test<true>(lo, hi, r, best_t, &e, slack, narrow && ref_sph[idx] == 0, gw)) continue;
    const int left = as_int(lo.w), right = as_int(hi.w);
    if (left < 0) {
      prim_test<false, false>(a.prims, left, r, best_t, best, c_tri, c_sph);
      if (right != left) prim_test<false, false>(a.prims, right, r, best_t, best, c_tri, c_sph);
    } else if (sp + 2 <= cap) {
      const StackT v[2] = {(StackT)right, (StackT)left};
#pragma unroll
      for (uint32_t j = 0; j < 2; ++j) {
        if (sp + j < rows) stk[(sp + j) * kBlock] = v[j];
        else ovf[(size_t)(sp + j - rows) * a.n_lanes] = v[j];
      }
      sp += 2;
    } else {
      atomicOr(ra->error_flag, kErrOverflow);
    }
  }
}


// BINARY's node test: the narrowed test with the grazing slack against tb, or,
// for a node whose subtree holds a sphere (KArgs::ref_sph), the reference's loose
// test against t_max = +inf: the rounded sphere test reaches beyond the sphere
// and its box by ~sqrt(u) |oc| and errs by as much in t (DESIGN.md §3 "Spheres").
__device__ __forceinline__ bool binary_test(const KArgs& a, int idx, const float4 lo, const float4 hi, const RayT& r,
                                            float tb, float* e, float slack, float gw) {
  if (a.ref_sph[idx]) return box_test<true>(lo, hi, r, __builtin_inff(), e, 0.0f, false);
  return box_test<true>(lo, hi, r, tb, e, slack, true, gw);
}

// Closest hit over the BVH.  FAST: near-first order with the narrowed slab
// test; REFERENCE: left-first DFS with exactly bvh.zig:187-205's tests.
template <bool FAST, bool STATS, class StackT>
__device__ __forceinline__ void traverse_bvh(const KArgs& a, const RayT& r, StackT* __restrict__ stk,
                                             float& best_t, int& best, uint32_t& c_nodes,
                                             uint32_t& c_tri, uint32_t& c_sph, ExcessAcc* excess = nullptr) {
  const int stride = kBlock;
  uint32_t sp = 0;
  const uint32_t cap = a.stack_depth;
  if (FAST) {
    const float slack = ray_slack(r, a.scene_extent, ray_m(r));
    const float gw = r.gk > 0.0f ?guard_grow(a, r) : 0.0f;  // the grazing-triangle guard
    float e;
    float4 lo = a.nodes[0], hi = a.nodes[1];
    if (STATS) ++c_nodes;
    if (!binary_test(a, 0, lo, hi, r, __builtin_fabsf(best_t) * kOpen + slack, &e, slack, gw)) {
      if (!ray_origin_ok(a, r)) reference_replay<StackT>(a, r, stk, 0u, best_t, best, false);
      return;
    }
    int left = as_int(lo.w), right = as_int(hi.w);
    for (;;) {
      if (left < 0) {
        prim_test<true, STATS, true>(a.prims, left, r, best_t, best, c_tri, c_sph);
        if (right != left) prim_test<true, STATS, true>(a.prims, right, r, best_t, best, c_tri, c_sph);
      } else {
        const float4 l0 = a.nodes[2 * left], l1 = a.nodes[2 * left + 1];
        const float4 r0 = a.nodes[2 * right], r1 = a.nodes[2 * right + 1];
        if (STATS) c_nodes += 2;
        const float tb = __builtin_fabsf(best_t) * kOpen + slack;
        float el, er;
        const bool hl = binary_test(a, left, l0, l1, r, tb, &el, slack, gw);
        const bool hr = binary_test(a, right, r0, r1, r, tb, &er, slack, gw);
        if (hl && hr) {
          const bool rfirst = er < el;
          const int far_idx = rfirst ? left : right;
          if (sp < cap) stk[(sp++) * stride] = (StackT)far_idx;
          else atomicOr(a.error_flag, kErrOverflow);  // too deep for the stack: the subtree is dropped (flagged)
          left = rfirst ? as_int(r0.w) : as_int(l0.w);
          right = rfirst ? as_int(r1.w) : as_int(l1.w);
          continue;
        }
        if (hl) { left = as_int(l0.w); right = as_int(l1.w); continue; }
        if (hr) { left = as_int(r0.w); right = as_int(r1.w); continue; }
      }
      // pop: re-test the node's own box against the (possibly shrunk) best_t
      bool found = false;
      while (sp > 0) {
        --sp;
        const int idx = stk[sp * stride];
        const float4 p0 = a.nodes[2 * idx], p1 = a.nodes[2 * idx + 1];
        if (STATS) ++c_nodes;
        if (binary_test(a, idx, p0, p1, r, __builtin_fabsf(best_t) * kOpen + slack, &e, slack, gw)) {
          left = as_int(p0.w);
          right = as_int(p1.w);
          found = true;
          break;
        }
      }
      if (!found) break;
    }
    // the order hazard of DESIGN.md §3, as in traverse_wide (the stack is all in LDS here)
    if (__builtin_expect(order_hazard<true>(a, r, best_t, best), 0))
      reference_replay<StackT>(a, r, stk, 0u, best_t, best);
    if (__builtin_expect(!ray_origin_ok(a, r), 0)) reference_replay<StackT>(a, r, stk, 0u, best_t, best, false);
  } else {
    stk[0] = 0;
    sp = 1;
    while (sp > 0) {
      --sp;
      const int idx = stk[sp * stride];
      const float4 lo = a.nodes[2 * idx], hi = a.nodes[2 * idx + 1];
      if (STATS) ++c_nodes;
      float e;
      if (!box_test<false>(lo, hi, r, best_t, &e)) continue;
      const int left = as_int(lo.w), right = as_int(hi.w);
      if (left < 0) {
        if (STATS && excess) excess->leaf(a.prims, lo, hi, r, left, right);
        prim_test<false, STATS>(a.prims, left, r, best_t, best, c_tri, c_sph);
        if (right != left) prim_test<false, STATS>(a.prims, right, r, best_t, best, c_tri, c_sph);
      } else {
        if (sp + 2 <= cap) {
          stk[sp * stride] = (StackT)right;
          stk[(sp + 1) * stride] = (StackT)left;
          sp += 2;
        } else {
          atomicOr(a.error_flag, kErrOverflow);
        }
      }
    }
  }
}

// Slab test of child slot k of a wide node: entry distance, or +inf on a miss.
// Every slot gets the narrowed test (entry > exit * (1 + 2^-16) culls; it never
// rejects a box holding a hit closer than best_t).  A leaf slot additionally
// gets the reference's own loose test (aabb.zig:109-127: each axis on its own
// against [t_min, t_max]) - its box is the reference leaf's box bit for bit.
__device__ __forceinline__ float wide_slot(float mnx, float mny, float mnz, float mxx, float mxy, float mxz,
                                           const RayT& r, float tb, bool leaf) {
  const float t_min = 0.001f;
  float a0 = (mnx - r.ox) * r.ix, a1 = (mxx - r.ox) * r.ix;
  float b0 = (mny - r.oy) * r.iy, b1 = (mxy - r.oy) * r.iy;
  float c0 = (mnz - r.oz) * r.iz, c1 = (mxz - r.oz) * r.iz;
  if (r.ix < 0.0f) { const float t = a0; a0 = a1; a1 = t; }
  if (r.iy < 0.0f) { const float t = b0; b0 = b1; b1 = t; }
  if (r.iz < 0.0f) { const float t = c0; c0 = c1; c1 = t; }
  // math.max(t0, t_min) / math.min(t1, t_max) are `x > y ? x : y` / `x < y ? x : y`;
  // with a non-NaN second operand these equal maxNum / minNum for every first
  // operand (a NaN slab bound, (bound - o) * inf with bound == o, then
  // constrains nothing, as in the reference) up to the sign of a zero result,
  // which no comparison below sees.
  const float an = __builtin_fmaxf(a0, t_min), ax = __builtin_fminf(a1, tb);
  const float bn = __builtin_fmaxf(b0, t_min), bx = __builtin_fminf(b1, tb);
  const float cn = __builtin_fmaxf(c0, t_min), cx = __builtin_fminf(c1, tb);
  const float en = __builtin_fmaxf(__builtin_fmaxf(an, bn), cn);
  const float ex = __builtin_fminf(__builtin_fminf(ax, bx), cx);
  bool ok = !(en > ex * ray_rel(r, ray_m(r)));
  if (leaf) ok = ok && (ax > an) && (bx > bn) && (cx > cn);  // !(tmax <= tmin) per axis
  return ok ? en : __builtin_inff();
}

__device__ __forceinline__ void cswap(float& ka, int& ra, float& kb, int& rb) {
  const bool s = kb < ka;
  const float tk = s ? kb : ka;
  const int tr = s ? rb : ra;
  kb = s ? ka : kb;
  rb = s ? ra : rb;
  ka = tk;
  ra = tr;
}

// Two slots' slab distances.  (Written as packed f32, v_pk_add_f32 /
// v_pk_mul_f32 with the same roundings, this traversal ran 1.2-1.8x slower:
// packed f32 issues at half the rate of single f32 here.)
typedef float f2 __attribute__((ext_vector_type(2)));

// The reference's (plane - o) * (1/d) as fma(plane, 1/d, -o/d): one rounding
// after an exact product instead of two, 24 VALU fewer
// per wide node.  With p = RN(o_k / d_k) such a distance lies within
// 1.0002 u |p| + 3.0001 u |s| of the reference's RN(RN(plane - o) * (1/d))
// (u = 2^-24); wide_iter's culls carry kFmaE2 * max_k |p_k| more slack for it
// (both ends of an interval), the relative margin (>= 2^-16) covers the rest, and
// each decision that must be the reference's own - a leaf's loose test, a sphere
// slot's static test, the hazard entry - is taken from these values only when it
// is certain by that margin (kFmaSure), else from the exact distances recomputed
// from memory (loose_slot / static_ok_slot), as for intervals within the margin.
// A ray with |1/d_k| >= 2^100 or |p_k| >= 2^120 (a direction component ~0) is
// "degenerate": it culls everything here and is traced the reference's way
// (wide_finish, ray_degenerate).
constexpr float kFmaE2 = 0x1.04p-23f;   // >= 2 x 1.0002 u (+ the rounding of this product)
constexpr float kFmaSure = 1.0000019f;  // 1 + 2^-19 > 1 + 6.0002 u: relative error of both ends
__device__ __forceinline__ f2 slab2f(float b0, float b1, float p, float inv) {
  return (f2){__builtin_fmaf(b0, inv, -p), __builtin_fmaf(b1, inv, -p)};
}
__device__ __forceinline__ bool ray_degenerate(const RayT& r) {
  const float pm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(r.ox * r.ix), __builtin_fabsf(r.oy * r.iy)),
                                   __builtin_fabsf(r.oz * r.iz));
  return !(ray_m(r) < 0x1p100f) || !(pm < 0x1p120f);
}

struct SlotT {
  float en, ex;
};
__device__ __forceinline__ SlotT slot_interval(float nx, float ny, float nz, float fx, float fy, float fz,
                                               float tb) {
  const float t_min = 0.001f;
  SlotT s;
  s.en = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, t_min));
  s.ex = __builtin_fminf(__builtin_fminf(fx, fy), __builtin_fminf(fz, tb));
  return s;
}
// The wide-tree encoding these kernels decode (accel_build.hpp kLayout*); the
// host refuses any other before launching, and a kernel handed one anyway sets
// kErrLayout and returns without reading the tree.
constexpr uint32_t kKernelLayout = kLayoutVersion | kLayoutSphereSlots | kLayoutSphereFirst;
__device__ __forceinline__ bool layout_ok(const KArgs& a) {
  if (a.layout == kKernelLayout) return true;  // (block-uniform: every thread returns together)
  if (threadIdx.x == 0) atomicOr(a.error_flag, kErrLayout);
  return false;
}
// The reference's loose test (aabb.zig:109-127) with t_max = +inf: every axis's
// (post-swap) slab [n, f] reaches past t_min and is not empty.  max(n, t_min) /
// min(f, +inf) as maxNum / minNum: a NaN bound constrains nothing, as math.max /
// math.min with t_min / t_max leave it in the reference.
__device__ __forceinline__ bool static_ok(float nx, float ny, float nz, float fx, float fy, float fz) {
  const float t_min = 0.001f, inf = __builtin_inff();
  return (__builtin_fminf(fx, inf) > __builtin_fmaxf(nx, t_min)) && (__builtin_fminf(fy, inf) > __builtin_fmaxf(ny, t_min)) &&
         (__builtin_fminf(fz, inf) > __builtin_fmaxf(nz, t_min));
}

// The reference's own loose test (aabb.zig:109-127) of leaf slot k whose
// narrowed test passed with en >= ex (rare; with en < ex it passes outright:
// an <= en < ex <= ax on every axis): each axis on its own, its distances
// recomputed from the node in memory (the same two roundings as the packed
// form) so that none of them stays live across the node.
// gg: the grazing-triangle guard's spatial widening of this ray (0: off), added to
// the leaf's own slack in both tests; the entry stays the exact loose entry, so a
// best hit found below it (a leaf opened only by the widening) is replayed.
// (planes: the slot's near / far planes in the ray's octant, bx / by / bz near, cx / cy / cz far)
__device__ __forceinline__ bool loose_planes(float bx, float by, float bz, float cx, float cy, float cz, const RayT& r,
                                             float tb, float& entry, float gg = 0.0f) {
  const float t_min = 0.001f;
  const float nx = (bx - r.ox) * r.ix, fx = (cx - r.ox) * r.ix;
  const float ny = (by - r.oy) * r.iy, fy = (cy - r.oy) * r.iy;
  const float nz = (bz - r.oz) * r.iz, fz = (cz - r.oz) * r.iz;
  // the exact loose entry (the order-hazard test's E; wide_iter's en when its slabs are not widened)
  entry = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, t_min));
  // the leaf's own coordinate slack (ray_slack): g = 2 x 2^-19 x its largest |coordinate|,
  // g |1/d_k| on axis k; a hit below the leaf's entry by that still counts against tb
  const float cl = __builtin_fmaxf(
      __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(bx), __builtin_fabsf(cx)),
                      __builtin_fmaxf(__builtin_fabsf(by), __builtin_fabsf(cy))),
      __builtin_fmaxf(__builtin_fabsf(bz), __builtin_fabsf(cz)));
  const float g = __builtin_fmaf(cl, r.gm, gg);
  const float gx = paxis_t(g, r.ix), gy = paxis_t(g, r.iy), gz = paxis_t(g, r.iz);
  const float tl = tb + __builtin_fmaxf(__builtin_fmaxf(gx, gy), gz);
  const bool loose = (__builtin_fminf(fx, tl) > __builtin_fmaxf(nx, t_min)) &&
                     (__builtin_fminf(fy, tl) > __builtin_fmaxf(ny, t_min)) &&
                     (__builtin_fminf(fz, tl) > __builtin_fmaxf(nz, t_min));
  // the narrowed test of the box grown by g (NaN bounds constrain nothing)
  const float en = __builtin_fmaxf(__builtin_fmaxf(nx - gx, ny - gy), __builtin_fmaxf(nz - gz, t_min));
  const float ex = __builtin_fminf(__builtin_fminf(fx + gx, fy + gy), __builtin_fminf(fz + gz, tl));
  return loose && !(en > ex * ray_rel(r, ray_m(r)));
}
__device__ __forceinline__ bool loose_slot(const float4* __restrict__ q, int k, const RayT& r, float tb,
                                           float& entry, float gg = 0.0f) {
  const float* f = reinterpret_cast<const float*>(q) + k;
  return loose_planes(f[0], f[4], f[8], f[12], f[16], f[20], r, tb, entry, gg);
}

// static_ok of leaf slot k, its slab distances recomputed from the node in memory
// (the same two roundings as wide_iter's) so that none stays live across the node
template <class FP>
__device__ __forceinline__ bool static_ok_at(FP f, const RayT& r, float& entry) {
  const float nx = (f[0] - r.ox) * r.ix, ny = (f[4] - r.oy) * r.iy, nz = (f[8] - r.oz) * r.iz;
  entry = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, 0.001f));  // the exact loose entry
  return static_ok(nx, ny, nz, (f[12] - r.ox) * r.ix, (f[16] - r.oy) * r.iy, (f[20] - r.oz) * r.iz);
}
// (q is a generic pointer: a node of the top levels lives in LDS - the root,
// which holds the ground sphere's leaf in every reference scene - and is read
// with ds_read, not a flat load through the vector memory path)
__device__ __forceinline__ bool static_ok_slot(const float4* __restrict__ q, int k, const RayT& r, float& entry) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (__builtin_amdgcn_is_shared(reinterpret_cast<const void*>(q)))
    return static_ok_at((const __attribute__((address_space(3))) float*)(reinterpret_cast<const float*>(q)) + k, r,
                        entry);
#endif
  return static_ok_at(reinterpret_cast<const float*>(q) + k, r, entry);
}

constexpr uint32_t kOctCopies = 8u;  // the wide tree is stored once per ray octant

// The wide tree's top levels (accel_build.cpp stores them first: nodes 0 ..
// n_top-1), every octant copy, copied into the block's LDS once at kernel
// start.  Every ray begins at the root and most go on to a level-1 node, and
// vector-memory data return (TD) is what the FAST loop saturates:
// these node reads come from LDS instead.  All threads of the block call this.
__device__ __forceinline__ void fill_lds_top(const KArgs& a, float4* __restrict__ top) {
  const uint32_t per = a.n_top * a.node_f4;  // float4 per octant copy
  for (uint32_t i = threadIdx.x; i < per * kOctCopies; i += kBlock) {
    const uint32_t o = i / per, j = i - o * per;
    top[i] = a.wnodes[o * a.wide_stride + j];
  }
  __syncthreads();
}

// The material table (a few records in every reference scene) copied into
// LDS at kernel start: the shading of a hit reads its material right after its
// shade record, a dependent chain of loads.
__device__ __forceinline__ void fill_lds_mats(const KArgs& a, float4* __restrict__ m) {
  const float4* src = reinterpret_cast<const float4*>(a.mats);
  for (uint32_t i = threadIdx.x; i < a.n_mats * 3u; i += kBlock) m[i] = src[i];
  __syncthreads();
}

// FAST: near-first over the 4-wide tree (accel_build.cpp), stored once per
// ray octant with each axis' min / max planes swapped where the octant's
// direction is negative, so a node's first three float4 are the four slots'
// near planes and the next three their far planes: the reference's swap
// (aabb.zig:116-118) is done by the layout, not per slot.  All four slots are
// tested against the t_max at node entry (a leaf passing with a t_max >= the
// current one is a superset of what the reference opens, and every primitive
// test still uses the current best with lower-slot tie-breaking); leaf slots
// are intersected in place, inner slots are sorted by entry distance and the
// farther ones pushed, branch-free.
// STATS: coherence of the FAST loop's fetches (kGlobalNodes .. kUniformPrims)
struct Coh {
  uint32_t gnodes = 0, unodes = 0, ptests = 0, uprims = 0, attw = 0, attr = 0, ovfw = 0;
  // wave-level events (kVNodeTrips ..), counted in the wave's first active lane
  uint32_t vn_trips = 0, vn_lines = 0, sn_trips = 0, rb_trips = 0, vp_trips = 0, vp_lines = 0, sp_trips = 0;
  uint32_t vsh_trips = 0, attw_trips = 0, attr_trips = 0, vn_cost = 0, vp_cost = 0;
  __device__ __forceinline__ void flush(unsigned long long* counters);
};

// STATS helpers: 1 in the first active lane of the wave (a wave-level event is
// counted once), and the number of distinct values of x among the active lanes
__device__ __forceinline__ uint32_t wave_once() {
  return __lane_id() == (uint32_t)__builtin_ctzll(__ballot(1)) ? 1u : 0u;
}
__device__ __forceinline__ uint32_t wave_distinct(uint32_t x) {
  uint64_t m = __ballot(1);
  uint32_t n = 0;
  while (m != 0ull) {
    const uint32_t f = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)__builtin_ctzll(m));
    m &= ~__ballot(x == f);
    ++n;
  }
  return n;
}

// One wide node's record in registers: the four slots' near planes, far planes
// (per axis, pre-swapped in the ray's octant copy) and primitive/child refs.
struct WideNode {
  float4 nx, ny, nz, fx, fy, fz, ra;
};

// (the octant's signs: unused - the planes come pre-swapped in the ray's octant copy -
// but dropping the arguments, dead as they are, changes how the lockstep kernel is scheduled)
__device__ __forceinline__ void wide_load(const float4* __restrict__ q, bool sx, bool sy, bool sz, WideNode& w) {
  (void)sx; (void)sy; (void)sz;
  w.nx = q[0]; w.ny = q[1]; w.nz = q[2]; w.fx = q[3]; w.fy = q[4]; w.fz = q[5]; w.ra = q[6];
}

// Where a ray reads the wide tree: its octant's copy (global memory) and that
// copy's top levels in LDS.
struct WideView {
  const float4* __restrict__ top;  // this octant's copy of the top nodes in LDS
  uint32_t base;                   // float4 offset of this octant's copy (< 2^32)
  uint32_t n_top;
};
// (the octant's three sign masks are no part of it: only the compressed nodes'
// leaf records read them, and form them there - OctSigns - instead of carrying them)
struct OctSigns {
  bool sx, sy, sz;
  __device__ __forceinline__ explicit OctSigns(const RayT& r) : sx(r.ix < 0.0f), sy(r.iy < 0.0f), sz(r.iz < 0.0f) {}
};

// oct * n for an octant (< 8) and a float4 count the host keeps below 2^24
// (zrt::check_octant_offsets): the product is below 2^27, exact in either form.
// A full-rate 24-bit multiply (v_mul_u32_u24) instead of the quarter-rate v_mul_lo_u32.
__device__ __forceinline__ uint32_t oct_times(uint32_t oct, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(oct, n);
#else
  return oct * n;
#endif
}

__device__ __forceinline__ WideView wide_view(const KArgs& a, const RayT& r, const float4* __restrict__ lds_top) {
  WideView v;
  const OctSigns s(r);
  const uint32_t oct = (s.sx ? 1u : 0u) | (s.sy ? 2u : 0u) | (s.sz ? 4u : 0u);
  v.base = oct_times(oct, a.wide_stride);
  v.top = lds_top + oct_times(oct, a.n_top * a.node_f4);
  v.n_top = a.n_top;
  return v;
}

// The address of wide node `i` for this ray: LDS for a top-level node, else
// its octant copy in global memory.
__device__ __forceinline__ const float4* wide_node_ptr(const KArgs& a, const WideView& v, uint32_t i) {
  return i < v.n_top ? v.top + 8u * i : a.wnodes + (v.base + 8u * i);
}

// FAST: near-first over the 4-wide tree (accel_build.cpp), stored once per
// ray octant with each axis' min / max planes swapped where the octant's
// direction is negative, so a node's first three float4 are the four slots'
// near planes and the next three their far planes: the reference's swap
// (aabb.zig:116-118) is done by the layout, not per slot.  All four slots are
// tested against the t_max at node entry (a leaf passing with a t_max >= the
// current one is a superset of what the reference opens, and every primitive
// test still uses the current best with lower-slot tie-breaking); leaf slots
// are intersected in place, inner slots are sorted by entry distance and the
// farther ones pushed, branch-free.
//
// wide_iter processes the node in `w` (read from q), picks the next node
// (pushing the farther inner children), intersects the opened leaves and loads
// the next node into `w` / q.  Returns false when the traversal is over (then
// the order-hazard test of wide_finish follows).  Its state between calls is
// (w, q, sp, best_t, best) and the lane's stack column, so a traversal can be
// suspended between nodes (the wavefront loop, render_loop_wf).
// SCALAR_NODES: a node every active lane reads next comes through the scalar cache
// (false in the wavefront and path-pool loops, whose lanes traverse unrelated nodes).
template <bool STATS, class StackT, bool SCALAR_NODES = true, bool PAXIS = false, bool GUARD = true>
__device__ __forceinline__ bool wide_iter(const KArgs& a, const RayT& r, const WideView& v,
                                          StackT* __restrict__ stk, uint32_t gl, WideNode& w,
                                          const float4*& q, uint32_t& sp, float& best_t, int& best,
                                          uint32_t& c_nodes, uint32_t& c_leaves, uint32_t& c_tri, uint32_t& c_sph,
                                          Coh& coh) {
  const int stride = kBlock;
  const uint32_t cap = a.stack_depth;  // rows allocated: the deepest push + 3
  // the first rows in LDS, the rest in global memory (a.lds_rows: zrt::plan_lds)
  constexpr bool kOvf = true;
  const uint32_t rows = a.lds_rows;
  const float inf = __builtin_inff();
  const OctSigns os(r);  // (wide_load)
  const bool sx = os.sx, sy = os.sy, sz = os.sz;
  int r0 = as_int(w.ra.x), r1 = as_int(w.ra.y), r2 = as_int(w.ra.z), r3 = as_int(w.ra.w);
  const float tb = __builtin_fabsf(best_t) * kOpen;
  const float m = ray_m(r), rel = ray_rel(r, m), slk = ray_slack(r, a.scene_extent, m);
  // slab distances fma(plane, 1/d, -p), p = o / d (see slab2f): E2 covers their error
  const float px = r.ox * r.ix, py = r.oy * r.iy, pz = r.oz * r.iz;
  const float pm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(px), __builtin_fabsf(py)), __builtin_fabsf(pz));
  const bool deg = !(m < 0x1p100f) || !(pm < 0x1p120f);  // ray_degenerate: nothing opens, wide_finish replays
  float E2 = pm * kFmaE2;
  // The grazing-triangle guard (DESIGN.md §3 "Triangles"): every box widened on
  // every axis by the reach g of the rounded triangle test, as w_k = g |1/d_k| in
  // t, through the offsets of the FMA form (near planes - (p + w), far planes
  // - (p - w)): no instruction per plane.  The exact interval then lies within
  // [en, en + wm] .. [ex - wm, ex], so certain decisions need 2 wm more (Eg).
  // (Two copies of the 24 distances under a scene-uniform branch: the offsets
  // held across one copy cost the lockstep kernel 11 more spilled VGPRs.)
  float Eg = E2, gg = 0.0f;  // gg: the guard's spatial widening (loose_slot), 0 when off
  f2 nx01, nx23, ny01, ny23, nz01, nz23, fx01, fx23, fy01, fy23, fz01, fz23;
#define ZRT_SLABS(PNX, PNY, PNZ, PFX, PFY, PFZ)                                                         \
  nx01 = slab2f(w.nx.x, w.nx.y, PNX, r.ix); nx23 = slab2f(w.nx.z, w.nx.w, PNX, r.ix);                   \
  ny01 = slab2f(w.ny.x, w.ny.y, PNY, r.iy); ny23 = slab2f(w.ny.z, w.ny.w, PNY, r.iy);                   \
  nz01 = slab2f(w.nz.x, w.nz.y, PNZ, r.iz); nz23 = slab2f(w.nz.z, w.nz.w, PNZ, r.iz);                   \
  fx01 = slab2f(w.fx.x, w.fx.y, PFX, r.ix); fx23 = slab2f(w.fx.z, w.fx.w, PFX, r.ix);                   \
  fy01 = slab2f(w.fy.x, w.fy.y, PFY, r.iy); fy23 = slab2f(w.fy.z, w.fy.w, PFY, r.iy);                   \
  fz01 = slab2f(w.fz.x, w.fz.y, PFZ, r.iz); fz23 = slab2f(w.fz.z, w.fz.w, PFZ, r.iz);
  // (the wavefront, path-pool and trace loops only: in the lockstep kernel the branch
  // alone cost 4 more spilled VGPRs, C4 -4 %, profiles/r04/r04d)
  if (GUARD && PAXIS && __builtin_expect(r.gk > 0.0f, 0)) {  // scene-uniform: a scalar branch
    const float g = guard_grow(a, r);
    gg = g;
    const float wx = paxis_t(g, r.ix), wy = paxis_t(g, r.iy), wz = paxis_t(g, r.iz);
    const float wm = __builtin_fmaxf(__builtin_fmaxf(wx, wy), wz);
    E2 = (pm + wm) * kFmaE2;  // (the offsets p -+ w are rounded too)
    Eg = __builtin_fmaf(wm, 2.0f, E2);
    ZRT_SLABS(px + wx, py + wy, pz + wz, px - wx, py - wy, pz - wz)
  } else {
    ZRT_SLABS(px, py, pz, px, py, pz)
  }
#undef ZRT_SLABS
  // a lane of the wave runs nearly parallel to an axis (paxis_grow): every slab
  // widened in place by its axis's own term; the leaf slots' exact intervals (the
  // reference's loose test, the hazard entry) are then recomputed by loose_slot
  bool pw = false;
  if (PAXIS && __builtin_expect(__ballot(m > a.paxis_m) != 0ull, 0)) {
    pw = true;
    const float g = paxis_grow(a, r);
    const float gx = paxis_t(g, r.ix), gy = paxis_t(g, r.iy), gz = paxis_t(g, r.iz);
    nx01.x -= gx; nx01.y -= gx; nx23.x -= gx; nx23.y -= gx;
    ny01.x -= gy; ny01.y -= gy; ny23.x -= gy; ny23.y -= gy;
    nz01.x -= gz; nz01.y -= gz; nz23.x -= gz; nz23.y -= gz;
    fx01.x += gx; fx01.y += gx; fx23.x += gx; fx23.y += gx;
    fy01.x += gy; fy01.y += gy; fy23.x += gy; fy23.y += gy;
    fz01.x += gz; fz01.y += gz; fz23.x += gz; fz23.y += gz;
  }
  SlotT s0 = slot_interval(nx01.x, ny01.x, nz01.x, fx01.x, fy01.x, fz01.x, tb);
  SlotT s1 = slot_interval(nx01.y, ny01.y, nz01.y, fx01.y, fy01.y, fz01.y, tb);
  SlotT s2 = slot_interval(nx23.x, ny23.x, nz23.x, fx23.x, fy23.x, fz23.x, tb);
  SlotT s3 = slot_interval(nx23.y, ny23.y, nz23.y, fx23.y, fy23.y, fz23.y, tb);
  // narrowed test: entry > exit * rel (+ slack for a leaf slot) culls (ray_slack:
  // inner slots' boxes are stored grown, leaf slots' are the reference leaves');
  // widened slabs carry their margins already (rounding: 2^-16)
  const float rl = pw ? 1.0000153f : rel, sl = (pw ? 0.0f : slk) + E2;
  const bool h0 = !deg && !(s0.en > __builtin_fmaf(s0.ex, rl, r0 < 0 ? sl : E2));
  const bool h1 = !deg && !(s1.en > __builtin_fmaf(s1.ex, rl, r1 < 0 ? sl : E2));
  const bool h2 = !deg && !(s2.en > __builtin_fmaf(s2.ex, rl, r2 < 0 ? sl : E2));
  const bool h3 = !deg && !(s3.en > __builtin_fmaf(s3.ex, rl, r3 < 0 ? sl : E2));
  if (STATS) {
    ++c_nodes;
    c_leaves += (r0 < 0) + (r1 < 0) + (r2 < 0) + (r3 < 0);
  }
  // leaf slots that pass both tests: their primitive refs (a in r_k, b in the node's last float4)
  bool o0 = r0 < 0 && h0, o1 = r1 < 0 && h1, o2 = r2 < 0 && h2, o3 = r3 < 0 && h3;
  // (certain: en < ex by the FMA distances' error)
#define ZRT_SURE(S) (__builtin_fmaf(S.en, kFmaSure, Eg) < S.ex)
  // (guarded: the slabs are widened, so every opened leaf takes its exact loose entry - the
  // hazard test's E - and its widened per-axis tests from memory)
  const bool pg = pw || gg > 0.0f;
  const bool w0 = o0 && (pg || !ZRT_SURE(s0)), w1 = o1 && (pg || !ZRT_SURE(s1));
  const bool w2 = o2 && (pg || !ZRT_SURE(s2)), w3 = o3 && (pg || !ZRT_SURE(s3));
  if (w0 || w1 || w2 || w3) {  // rare: an interval within the margin, decide per axis
    if (w0) o0 = loose_slot(q, 0, r, tb, s0.en, gg);
    if (w1) o1 = loose_slot(q, 1, r, tb, s1.en, gg);
    if (w2) o2 = loose_slot(q, 2, r, tb, s2.en, gg);
    if (w3) o3 = loose_slot(q, 3, r, tb, s3.en, gg);
  }
  // leaf slots holding a sphere (ref a - 2^30, accel_build.hpp): opened when the
  // reference's loose test passes against t_max = +inf.  The rounded sphere test
  // accepts rays that pass outside the sphere - and its box - by up to ~sqrt(u)|oc|
  // and errs by as much in t (DESIGN.md §3 "Spheres"), so neither the narrowed
  // test nor the current best may cull them; every sphere hit of a static-ok
  // leaf is then seen, and the order-hazard tests see it too.  (A wave-uniform
  // branch: nodes with sphere leaves are few.)
  // The slot's interval in registers settles most: en < ex (the narrowed interval
  // is not empty: every axis passes) opens it, ex <= t_min (an axis's far plane
  // at or behind t_min: that axis fails; tb > t_min) keeps it shut; the rest, and
  // every slot of a widened wave (pw), take the per-axis test from memory.
  // (accel_build puts a node's sphere leaves in its first slots)
  if (__builtin_expect(__ballot(r0 < -kSphereSlotBias) != 0ull, 0)) {
#define ZRT_SPHERE_SLOT(K)                                                                                   \
  if (r##K < -kSphereSlotBias) {                                                                             \
    o##K = !pw && !deg && ZRT_SURE(s##K);                                                                    \
    if (!o##K && !deg && s##K.ex + __builtin_fmaf(__builtin_fabsf(s##K.ex), 0x1p-19f, Eg) > 0.001f)          \
      o##K = static_ok_slot(q, K, r, s##K.en);                                                               \
    r##K += kSphereSlotBias;                                                                                 \
  }
    ZRT_SPHERE_SLOT(0)
    ZRT_SPHERE_SLOT(1)
    ZRT_SPHERE_SLOT(2)
    ZRT_SPHERE_SLOT(3)
#undef ZRT_SPHERE_SLOT
  }
#undef ZRT_SURE
  const int l0 = o0 ? r0 : 0, l1 = o1 ? r1 : 0, l2 = o2 ? r2 : 0, l3 = o3 ? r3 : 0;
  const float4* leaf_q = q;  // (the leaves are intersected after the next node is chosen)
  int32_t next = -1;
  // inner slots that pass, keyed by entry distance
  float k0 = r0 >= 0 && h0 ? s0.en : inf, k1 = r1 >= 0 && h1 ? s1.en : inf;
  float k2 = r2 >= 0 && h2 ? s2.en : inf, k3 = r3 >= 0 && h3 ? s3.en : inf;
  const uint32_t n = (k0 != inf) + (k1 != inf) + (k2 != inf) + (k3 != inf);
  // every active lane's stack top and its next three pushes inside the LDS rows (a
  // wave-uniform test, true throughout for trees whose stack fits the LDS plan): the
  // same branches as the generic form below, the pop a ds_read of the lane's LDS
  // column - not a generic load that could also reach the global rows (C3 +1.6-2.4 %,
  // C4 +0.3 %: profiles/r06/r06w; push / pop as LDS selects instead: C3 +1.3 %, C4 ±0.3 %)
  if (__ballot(sp + 3u > rows) == 0ull) {
    if (__ballot(n > 1u) == 0ull) {
      if (n != 0) {
        next = k0 != inf ? r0 : k1 != inf ? r1 : k2 != inf ? r2 : r3;
      } else if (sp != 0) {
        --sp;
        next = (int32_t)stk[sp * stride];
      }
    } else {
      cswap(k0, r0, k1, r1);
      cswap(k2, r2, k3, r3);
      cswap(k0, r0, k2, r2);
      cswap(k1, r1, k3, r3);
      cswap(k1, r1, k2, r2);
      if (n != 0) {
        stk[sp * stride] = (StackT)(n == 4 ? r3 : n == 3 ? r2 : r1);
        stk[(sp + 1) * stride] = (StackT)(n == 4 ? r2 : r1);
        stk[(sp + 2) * stride] = (StackT)r1;
        const uint32_t nsp = sp + n - 1;
        if (__builtin_expect(nsp > cap - 3, 0)) raise_error(a, kErrOverflow);
        sp = min(nsp, cap - 3);
        next = r0;
      } else if (sp != 0) {
        --sp;
        next = (int32_t)stk[sp * stride];
      }
    }
  } else if (__ballot(n > 1u) == 0ull) {
    // every active lane follows at most one inner child: no sort, nothing to push
    // (a wave-uniform branch around the 5 compare-exchanges and the 3 stores)
    if (n != 0) {
      next = k0 != inf ? r0 : k1 != inf ? r1 : k2 != inf ? r2 : r3;
    } else if (sp != 0) {
      --sp;
      next = kOvf && sp >= rows ? (row_ok<STATS>(a, (uint64_t)(sp - rows) * a.n_lanes + gl, a.ovf_cap) ? (int32_t)ovf_column<StackT>(a, gl)[(size_t)(sp - rows) * a.n_lanes] : -1)
                                  : (int32_t)stk[sp * stride];
    }
  } else {
    // sort (entry, ref) ascending: 5 compare-exchanges
    cswap(k0, r0, k1, r1);
    cswap(k2, r2, k3, r3);
    cswap(k0, r0, k2, r2);
    cswap(k1, r1, k3, r3);
    cswap(k1, r1, k2, r2);
    if (n != 0) {
      // push r_{n-1} .. r_1 (farthest first) and continue with the nearest; the
      // three stores are unconditional (entries above the new top are dead)
      const StackT e0 = (StackT)(n == 4 ? r3 : n == 3 ? r2 : r1), e1 = (StackT)(n == 4 ? r2 : r1);
      const StackT e2 = (StackT)r1;
      // sp <= cap - 3 always holds (the clamp below), so the three stores stay in the rows
      if (sp + 3 <= rows) {
        stk[sp * stride] = e0;
        stk[(sp + 1) * stride] = e1;
        stk[(sp + 2) * stride] = e2;
      } else if (kOvf) {  // deep trees: rows past the LDS part live in global memory
        const StackT e[3] = {e0, e1, e2};
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
          if (sp + j < rows) {
            stk[(sp + j) * stride] = e[j];
          } else {
            if (row_ok<STATS>(a, (uint64_t)(sp + j - rows) * a.n_lanes + gl, a.ovf_cap))
              ovf_column<StackT>(a, gl)[(size_t)(sp + j - rows) * a.n_lanes] = e[j];
            if (STATS) ++coh.ovfw;
          }
        }
      }
      const uint32_t nsp = sp + n - 1;
      // the host sizes cap = the tree's deepest stack + 3, so this never fires
      // unless the stack was sized too small: then entries would be lost
      if (__builtin_expect(nsp > cap - 3, 0)) raise_error(a, kErrOverflow);
      sp = min(nsp, cap - 3);
      next = r0;
    } else if (sp != 0) {
      --sp;
      next = kOvf && sp >= rows ? (row_ok<STATS>(a, (uint64_t)(sp - rows) * a.n_lanes + gl, a.ovf_cap) ? (int32_t)ovf_column<StackT>(a, gl)[(size_t)(sp - rows) * a.n_lanes] : -1)
                                    : (int32_t)stk[sp * stride];
    }
  }
  // each lane walks ITS opened leaves in slot order, so lanes that opened
  // different slots share loop trips (the result is the closest t, ties to
  // the lower slot, order hazards flagged).  A/B against four unrolled slot
  // blocks: C5 +2.9 %, C3 +3.2 %, C4 -0.2 % (and one copy of the tests).
  uint32_t open = (l0 != 0 ? 1u : 0u) | (l1 != 0 ? 2u : 0u) | (l2 != 0 ? 4u : 0u) | (l3 != 0 ? 8u : 0u);
  if (open != 0) {
    // the second refs: a vector load even for a wave-uniform node (through the scalar
    // cache: exact, C4 -2.4 %, C3 -1.9 %, profiles/r06/r06o: less data-return work,
    // more issue)
    const float4 rb = leaf_q[7];
    if (STATS) coh.rb_trips += wave_once();
    do {
      const uint32_t k = (uint32_t)__builtin_ctz(open);
      open &= open - 1u;
      const int L = k == 0 ? l0 : k == 1 ? l1 : k == 2 ? l2 : l3;
      const int pb = as_int(k == 0 ? rb.x : k == 1 ? rb.y : k == 2 ? rb.z : rb.w);
      // the leaf's loose entry, or (FMA distances) an upper bound of it: flags a superset
      // (a guarded leaf's entry is exact: it went through loose_slot)
      const float lp = __builtin_fmaf(k == 0 ? s0.en : k == 1 ? s1.en : k == 2 ? s2.en : s3.en, kFmaSure, E2);
      if (STATS) {
        const int f = __builtin_amdgcn_readfirstlane(L);
        coh.ptests += 1u;
        coh.uprims += __ballot(L != f) == 0ull ? 1u : 0u;
      }
      const int fl = __builtin_amdgcn_readfirstlane(L), fb = __builtin_amdgcn_readfirstlane(pb);
      if (__ballot(L != fl || pb != fb) == 0ull) {  // one leaf in every active lane: scalar loads
        if (STATS) coh.sp_trips += wave_once() * (fb != fl ? 2u : 1u);
        prim_test_uniform<true, STATS, true>(a.prims, fl, r, best_t, best, c_tri, c_sph, lp);
        if (fb != fl) prim_test_uniform<true, STATS, true>(a.prims, fb, r, best_t, best, c_tri, c_sph, lp);
      } else {
        if (STATS) {
          const uint32_t dl = wave_distinct((uint32_t)L);
          if (wave_once()) { ++coh.vp_trips; coh.vp_lines += dl; coh.vp_cost += max(16u, dl); }
        }
        prim_test<true, STATS, true>(a.prims, L, r, best_t, best, c_tri, c_sph, lp);
        if (pb != L) {
          if (STATS) {
            const uint32_t db = wave_distinct((uint32_t)pb);
            if (wave_once()) { ++coh.vp_trips; coh.vp_lines += db; coh.vp_cost += max(16u, db); }
          }
          prim_test<true, STATS, true>(a.prims, pb, r, best_t, best, c_tri, c_sph, lp);
        }
      }
    } while (open != 0);
  }
  if (STATS && next >= 0 && (uint32_t)next >= v.n_top) {
    const int32_t f = __builtin_amdgcn_readfirstlane(next);
    const bool uni = __ballot(next != f || (uint32_t)next < v.n_top) == 0ull;  // (among the lanes here)
    ++coh.gnodes;
    coh.unodes += uni ? 1u : 0u;
  }
  if (next < 0) return false;
  if ((uint32_t)next < v.n_top) {  // a top-level node: from LDS (ds_read)
    const float4* __restrict__ t = v.top + 8u * (uint32_t)next;
    // (q naming the node's global copy even here, so that the leaf refs and the rare plane
    // re-reads never go through a generic pointer: exact, C4 -0.5 %, C3 +-0, profiles/r06/r06q2)
    q = t;
    wide_load(t, sx, sy, sz, w);
  } else {
    const uint32_t at = v.base + 8u * (uint32_t)next;  // this ray's octant copy
    const float4* __restrict__ g = a.wnodes + at;
    q = g;
    const uint32_t fa = __builtin_amdgcn_readfirstlane(at);
    if (SCALAR_NODES && __ballot(at != fa) == 0ull) {  // one node in every active lane: scalar loads
      if (STATS) coh.sn_trips += wave_once();
#if defined(__HIP_DEVICE_COMPILE__)
      typedef const __attribute__((address_space(4))) float4 cfloat4;
      wide_load(reinterpret_cast<const float4*>((cfloat4*)a.wnodes + fa), sx, sy, sz, w);
#else
      wide_load(a.wnodes + fa, sx, sy, sz, w);
#endif
    } else {
      if (STATS) {
        const uint32_t dn = wave_distinct(at);
        if (wave_once()) { ++coh.vn_trips; coh.vn_lines += dn; coh.vn_cost += max(16u, dn); }
      }
      wide_load(g, sx, sy, sz, w);
    }
  }
  return true;
}

// The end of a FAST traversal: the order hazard of DESIGN.md §3 (1e-8..1e-5
// of rays) re-traced the reference's way.
template <bool STATS, class StackT, bool LEAN = false>
__device__ __forceinline__ void wide_finish(const KArgs& a, const RayT& r, StackT* __restrict__ stk, uint32_t gl,
                                            float& best_t, int& best, uint32_t& c_replays) {
  // an origin farther out than the sphere growth was sized for: the reference's
  // way alone (narrow = false).  One call site for both cases: the replay is
  // inlined, and a second copy cost the lockstep loop 2.8 % on C4 (registers).
  // (the lean kernel is launched only where the host found check_origins 0)
  const bool far = __builtin_expect((!Lean<LEAN>::origin && !ray_origin_ok(a, r)) || ray_degenerate(r), 0);
  if (__builtin_expect(order_hazard<false>(a, r, best_t, best) || far, 0)) {
    if (STATS) ++c_replays;
    reference_replay<StackT>(a, r, stk, gl, best_t, best, !far);
  }
}

// ---------------------------------------------------------------------------
// Compressed wide nodes (accel_build.hpp quantize_wide; DESIGN.md §3
// "Compressed nodes"): 64 B per node - the origin and per-axis power-of-two
// step, the 24 planes as bytes, the refs - instead of 128 B, for trees past the
// caches (the C5 mesh: 475 MB of octant copies become 238 MB).  A plane decodes
// exactly (origin + q * step is an f32 by construction), so the slab distances
// and every margin are wide_iter's; the quantized boxes contain the full nodes'
// boxes, so the culls are supersets.  A leaf slot's exact box (the reference's,
// bit for bit) and its primitive refs come from its leaf record, read when the
// quantized box passes: every decision wide_iter takes from the leaf's planes -
// the narrowed and loose tests, a sphere slot's static test, the hazard entry -
// is taken from the record's planes with wide_iter's formulas.
struct WideNodeQ {
  float4 f0, f1, f2, f3;  // {origin.xyz, steps}, {near x/y/z, far x}, {far y/z, ref 0/1}, {ref 2/3, 0, 0}
};
template <class P>
__device__ __forceinline__ void qnode_load(P q, WideNodeQ& w) {
  w.f0 = q[0];
  w.f1 = q[1];
  w.f2 = q[2];
  w.f3 = q[3];
}
// plane byte k of `word`: origin + q * step (exact: a product of a byte and a
// power of two, then a sum the encoder made representable)
__device__ __forceinline__ float qplane(uint32_t word, int k, float step, float origin) {
  return __builtin_fmaf((float)((word >> (8 * k)) & 0xffu), step, origin);
}
__device__ __forceinline__ float qstep(uint32_t e8) { return __uint_as_float(e8 << 23); }

// static_ok (aabb.zig:109-127 against t_max = +inf) of a box given by its planes in
// the ray's octant, and its exact loose entry
__device__ __forceinline__ bool static_ok_planes(float bx, float by, float bz, float cx, float cy, float cz,
                                                 const RayT& r, float& entry) {
  const float nx = (bx - r.ox) * r.ix, ny = (by - r.oy) * r.iy, nz = (bz - r.oz) * r.iz;
  entry = __builtin_fmaxf(__builtin_fmaxf(nx, ny), __builtin_fmaxf(nz, 0.001f));
  return static_ok(nx, ny, nz, (cx - r.ox) * r.ix, (cy - r.oy) * r.iy, (cz - r.oz) * r.iz);
}

template <bool STATS, class StackT, bool PAXIS = true, bool GUARD = true>
__device__ __forceinline__ bool wide_iter_q(const KArgs& a, const RayT& r, const WideView& v,
                                            StackT* __restrict__ stk, uint32_t gl, WideNodeQ& w,
                                            const float4*& q, uint32_t& sp, float& best_t, int& best,
                                            uint32_t& c_nodes, uint32_t& c_leaves, uint32_t& c_tri, uint32_t& c_sph,
                                            Coh& coh) {
  (void)q;
  const int stride = kBlock;
  const uint32_t cap = a.stack_depth;
  const uint32_t rows = a.lds_rows;  // the first rows in LDS, the rest in global memory (either stack width)
  StackT* __restrict__ ovf = reinterpret_cast<StackT*>(a.stack_ovf) + gl;
  const float inf = __builtin_inff();
  const OctSigns os(r);  // (a leaf record holds the reference's box: its planes are picked per ray)
  const bool sx = os.sx, sy = os.sy, sz = os.sz;
  int r0 = as_int(w.f2.z), r1 = as_int(w.f2.w), r2 = as_int(w.f3.x), r3 = as_int(w.f3.y);
  const float ox = w.f0.x, oy = w.f0.y, oz = w.f0.z;
  const uint32_t ee = __float_as_uint(w.f0.w);
  const float stx = qstep(ee & 0xffu), sty = qstep((ee >> 8) & 0xffu), stz = qstep((ee >> 16) & 0xffu);
  const uint32_t bnx = __float_as_uint(w.f1.x), bny = __float_as_uint(w.f1.y), bnz = __float_as_uint(w.f1.z);
  const uint32_t bfx = __float_as_uint(w.f1.w), bfy = __float_as_uint(w.f2.x), bfz = __float_as_uint(w.f2.y);
  const float tb = __builtin_fabsf(best_t) * kOpen;
  const float m = ray_m(r), rel = ray_rel(r, m), slk = ray_slack(r, a.scene_extent, m);
  const float px = r.ox * r.ix, py = r.oy * r.iy, pz = r.oz * r.iz;
  const float pm = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(px), __builtin_fabsf(py)), __builtin_fabsf(pz));
  const bool deg = !(m < 0x1p100f) || !(pm < 0x1p120f);  // ray_degenerate: nothing opens, wide_finish replays
  float E2 = pm * kFmaE2;
  float Eg = E2, gg = 0.0f;
  // the slab offsets of the near / far planes (wide_iter: p -+ the guard's w)
  float onx = px, ony = py, onz = pz, ofx = px, ofy = py, ofz = pz;
  if (GUARD && PAXIS && __builtin_expect(r.gk > 0.0f, 0)) {  // scene-uniform: a scalar branch
    const float g = guard_grow(a, r);
    gg = g;
    const float wx = paxis_t(g, r.ix), wy = paxis_t(g, r.iy), wz = paxis_t(g, r.iz);
    const float wm = __builtin_fmaxf(__builtin_fmaxf(wx, wy), wz);
    E2 = (pm + wm) * kFmaE2;
    Eg = __builtin_fmaf(wm, 2.0f, E2);
    onx = px + wx; ony = py + wy; onz = pz + wz;
    ofx = px - wx; ofy = py - wy; ofz = pz - wz;
  }
#define ZRT_QSLAB(BW, K, ST, OR, OFF, INV) __builtin_fmaf(qplane(BW, K, ST, OR), INV, -(OFF))
  f2 nx01 = {ZRT_QSLAB(bnx, 0, stx, ox, onx, r.ix), ZRT_QSLAB(bnx, 1, stx, ox, onx, r.ix)};
  f2 nx23 = {ZRT_QSLAB(bnx, 2, stx, ox, onx, r.ix), ZRT_QSLAB(bnx, 3, stx, ox, onx, r.ix)};
  f2 ny01 = {ZRT_QSLAB(bny, 0, sty, oy, ony, r.iy), ZRT_QSLAB(bny, 1, sty, oy, ony, r.iy)};
  f2 ny23 = {ZRT_QSLAB(bny, 2, sty, oy, ony, r.iy), ZRT_QSLAB(bny, 3, sty, oy, ony, r.iy)};
  f2 nz01 = {ZRT_QSLAB(bnz, 0, stz, oz, onz, r.iz), ZRT_QSLAB(bnz, 1, stz, oz, onz, r.iz)};
  f2 nz23 = {ZRT_QSLAB(bnz, 2, stz, oz, onz, r.iz), ZRT_QSLAB(bnz, 3, stz, oz, onz, r.iz)};
  f2 fx01 = {ZRT_QSLAB(bfx, 0, stx, ox, ofx, r.ix), ZRT_QSLAB(bfx, 1, stx, ox, ofx, r.ix)};
  f2 fx23 = {ZRT_QSLAB(bfx, 2, stx, ox, ofx, r.ix), ZRT_QSLAB(bfx, 3, stx, ox, ofx, r.ix)};
  f2 fy01 = {ZRT_QSLAB(bfy, 0, sty, oy, ofy, r.iy), ZRT_QSLAB(bfy, 1, sty, oy, ofy, r.iy)};
  f2 fy23 = {ZRT_QSLAB(bfy, 2, sty, oy, ofy, r.iy), ZRT_QSLAB(bfy, 3, sty, oy, ofy, r.iy)};
  f2 fz01 = {ZRT_QSLAB(bfz, 0, stz, oz, ofz, r.iz), ZRT_QSLAB(bfz, 1, stz, oz, ofz, r.iz)};
  f2 fz23 = {ZRT_QSLAB(bfz, 2, stz, oz, ofz, r.iz), ZRT_QSLAB(bfz, 3, stz, oz, ofz, r.iz)};
#undef ZRT_QSLAB
  // per-axis widening (wide_iter, paxis_grow): the same terms, kept for the leaf records
  bool pw = false;
  float gx = 0.0f, gy = 0.0f, gz = 0.0f;
  if (PAXIS && __builtin_expect(__ballot(m > a.paxis_m) != 0ull, 0)) {
    pw = true;
    const float g = paxis_grow(a, r);
    gx = paxis_t(g, r.ix); gy = paxis_t(g, r.iy); gz = paxis_t(g, r.iz);
    nx01.x -= gx; nx01.y -= gx; nx23.x -= gx; nx23.y -= gx;
    ny01.x -= gy; ny01.y -= gy; ny23.x -= gy; ny23.y -= gy;
    nz01.x -= gz; nz01.y -= gz; nz23.x -= gz; nz23.y -= gz;
    fx01.x += gx; fx01.y += gx; fx23.x += gx; fx23.y += gx;
    fy01.x += gy; fy01.y += gy; fy23.x += gy; fy23.y += gy;
    fz01.x += gz; fz01.y += gz; fz23.x += gz; fz23.y += gz;
  }
  const SlotT s0 = slot_interval(nx01.x, ny01.x, nz01.x, fx01.x, fy01.x, fz01.x, tb);
  const SlotT s1 = slot_interval(nx01.y, ny01.y, nz01.y, fx01.y, fy01.y, fz01.y, tb);
  const SlotT s2 = slot_interval(nx23.x, ny23.x, nz23.x, fx23.x, fy23.x, fz23.x, tb);
  const SlotT s3 = slot_interval(nx23.y, ny23.y, nz23.y, fx23.y, fy23.y, fz23.y, tb);
  const float rl = pw ? 1.0000153f : rel, sl = (pw ? 0.0f : slk) + E2;
  // the quantized boxes' narrowed test (a superset of the full node's, with its margins)
  const bool h0 = !deg && !(s0.en > __builtin_fmaf(s0.ex, rl, r0 < 0 ? sl : E2));
  const bool h1 = !deg && !(s1.en > __builtin_fmaf(s1.ex, rl, r1 < 0 ? sl : E2));
  const bool h2 = !deg && !(s2.en > __builtin_fmaf(s2.ex, rl, r2 < 0 ? sl : E2));
  const bool h3 = !deg && !(s3.en > __builtin_fmaf(s3.ex, rl, r3 < 0 ? sl : E2));
  if (STATS) {
    ++c_nodes;
    c_leaves += (r0 < 0) + (r1 < 0) + (r2 < 0) + (r3 < 0);
  }
  // candidate leaf slots, decided against their records below: a triangle leaf whose
  // quantized box passes the narrowed test; a sphere leaf (wide_iter: opened by the
  // static test against t_max = +inf, never culled by the best) whose quantized exit
  // can lie past t_min (its exact exit is not larger)
#define ZRT_QCAND(K) \
  (r##K < 0 && r##K != kEmptyRef && \
   (r##K < -kSphereSlotBias ? !deg && s##K.ex + __builtin_fmaf(__builtin_fabsf(s##K.ex), 0x1p-19f, Eg) > 0.001f : h##K))
  uint32_t open = (ZRT_QCAND(0) ? 1u : 0u) | (ZRT_QCAND(1) ? 2u : 0u) | (ZRT_QCAND(2) ? 4u : 0u) |
                  (ZRT_QCAND(3) ? 8u : 0u);
#undef ZRT_QCAND
  const int l0 = r0, l1 = r1, l2 = r2, l3 = r3;
  int32_t next = -1;
  float k0 = r0 >= 0 && h0 ? s0.en : inf, k1 = r1 >= 0 && h1 ? s1.en : inf;
  float k2 = r2 >= 0 && h2 ? s2.en : inf, k3 = r3 >= 0 && h3 ? s3.en : inf;
  const uint32_t n = (k0 != inf) + (k1 != inf) + (k2 != inf) + (k3 != inf);
  if (__ballot(n > 1u) == 0ull) {
    if (n != 0) {
      next = k0 != inf ? r0 : k1 != inf ? r1 : k2 != inf ? r2 : r3;
    } else if (sp != 0) {
      --sp;
      next = sp >= rows ? (row_ok<STATS>(a, (uint64_t)(sp - rows) * a.n_lanes + gl, a.ovf_cap) ? (int32_t)ovf[(size_t)(sp - rows) * a.n_lanes] : -1)
                        : (int32_t)stk[sp * stride];
    }
  } else {
    cswap(k0, r0, k1, r1);
    cswap(k2, r2, k3, r3);
    cswap(k0, r0, k2, r2);
    cswap(k1, r1, k3, r3);
    cswap(k1, r1, k2, r2);
    if (n != 0) {
      const StackT e0 = (StackT)(n == 4 ? r3 : n == 3 ? r2 : r1), e1 = (StackT)(n == 4 ? r2 : r1);
      const StackT e2 = (StackT)r1;
      if (sp + 3 <= rows) {
        stk[sp * stride] = e0;
        stk[(sp + 1) * stride] = e1;
        stk[(sp + 2) * stride] = e2;
      } else {
        const StackT e[3] = {e0, e1, e2};
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
          if (sp + j < rows) {
            stk[(sp + j) * stride] = e[j];
          } else {
            if (row_ok<STATS>(a, (uint64_t)(sp + j - rows) * a.n_lanes + gl, a.ovf_cap))
              ovf[(size_t)(sp + j - rows) * a.n_lanes] = e[j];
            if (STATS) ++coh.ovfw;
          }
        }
      }
      const uint32_t nsp = sp + n - 1;
      if (__builtin_expect(nsp > cap - 3, 0)) atomicOr(a.error_flag, kErrOverflow);
      sp = min(nsp, cap - 3);
      next = r0;
    } else if (sp != 0) {
      --sp;
      next = sp >= rows ? (row_ok<STATS>(a, (uint64_t)(sp - rows) * a.n_lanes + gl, a.ovf_cap) ? (int32_t)ovf[(size_t)(sp - rows) * a.n_lanes] : -1)
                        : (int32_t)stk[sp * stride];
    }
  }
  // each lane walks its candidate leaves in slot order: the record's exact box
  // through wide_iter's leaf decisions, then the primitives
  while (open != 0) {
    const uint32_t k = (uint32_t)__builtin_ctz(open);
    open &= open - 1u;
    const int ref = k == 0 ? l0 : k == 1 ? l1 : k == 2 ? l2 : l3;
    const bool sph = ref < -kSphereSlotBias;
    const uint32_t L = (uint32_t)(-(sph ? ref + kSphereSlotBias : ref) - 1);
    if (__builtin_expect(L >= a.n_qleaves, 0)) {  // a corrupt ref: report, never read past the records
      atomicOr(a.error_flag, kErrLayout);
      continue;
    }
    const float4 mn = a.qleaves[2 * L], mx = a.qleaves[2 * L + 1];
    const float bx = sx ? mx.x : mn.x, cx = sx ? mn.x : mx.x;
    const float by = sy ? mx.y : mn.y, cy = sy ? mn.y : mx.y;
    const float bz = sz ? mx.z : mn.z, cz = sz ? mn.z : mx.z;
    // wide_iter's distances of this slot: the same planes, offsets and widening
    SlotT s = slot_interval(__builtin_fmaf(bx, r.ix, -onx) - gx, __builtin_fmaf(by, r.iy, -ony) - gy,
                            __builtin_fmaf(bz, r.iz, -onz) - gz, __builtin_fmaf(cx, r.ix, -ofx) + gx,
                            __builtin_fmaf(cy, r.iy, -ofy) + gy, __builtin_fmaf(cz, r.iz, -ofz) + gz, tb);
#define ZRT_SURE(S) (__builtin_fmaf(S.en, kFmaSure, Eg) < S.ex)
    // (in wide_iter's order: the narrowed test, the per-axis test within the margin,
    // then a sphere slot's static test, which decides it)
    bool o = !deg && !(s.en > __builtin_fmaf(s.ex, rl, sl));
    if (o && (pw || gg > 0.0f || !ZRT_SURE(s))) o = loose_planes(bx, by, bz, cx, cy, cz, r, tb, s.en, gg);
    if (sph) {
      o = !pw && !deg && ZRT_SURE(s);
      if (!o && !deg && s.ex + __builtin_fmaf(__builtin_fabsf(s.ex), 0x1p-19f, Eg) > 0.001f)
        o = static_ok_planes(bx, by, bz, cx, cy, cz, r, s.en);
    }
#undef ZRT_SURE
    if (!o) continue;
    const int La = as_int(mn.w), pb = as_int(mx.w);
    const float lp = __builtin_fmaf(s.en, kFmaSure, E2);
    if (STATS) {
      const int f = __builtin_amdgcn_readfirstlane(La);
      coh.ptests += 1u;
      coh.uprims += __ballot(La != f) == 0ull ? 1u : 0u;
    }
    prim_test<true, STATS, true>(a.prims, La, r, best_t, best, c_tri, c_sph, lp);
    if (pb != La) prim_test<true, STATS, true>(a.prims, pb, r, best_t, best, c_tri, c_sph, lp);
  }
  if (STATS && next >= 0 && (uint32_t)next >= v.n_top) {
    const int32_t f = __builtin_amdgcn_readfirstlane(next);
    const bool uni = __ballot(next != f || (uint32_t)next < v.n_top) == 0ull;
    ++coh.gnodes;
    coh.unodes += uni ? 1u : 0u;
  }
  if (next < 0) return false;
  if (__builtin_expect((uint32_t)next >= a.n_qnodes, 0)) {  // a corrupt node index: report, never read past the tree
    atomicOr(a.error_flag, kErrLayout);
    return false;
  }
  if ((uint32_t)next < v.n_top) {  // a top-level node: from LDS
    const float4* __restrict__ t = v.top + kQuantNodeF4 * (uint32_t)next;
    q = t;
    qnode_load(t, w);
  } else {
    const uint32_t at = v.base + kQuantNodeF4 * (uint32_t)next;
    const float4* __restrict__ g = a.wnodes + at;
    q = g;
    qnode_load(g, w);
  }
  return true;
}

// the suspended node of a wavefront / pool lane (re)loaded, in either format
template <bool QN, class W>
__device__ __forceinline__ void node_load(const float4* q, const RayT& r, W& w) {
  if constexpr (QN) {
    qnode_load(q, w);
  } else {
    const OctSigns os(r);
    wide_load(q, os.sx, os.sy, os.sz, w);
  }
}

// zrt_trace over compressed nodes (MODE 8): traverse_wide with wide_iter_q
template <bool STATS, class StackT>
__device__ __forceinline__ void traverse_wide_q(const KArgs& a, const RayT& r, StackT* __restrict__ stk,
                                                const float4* __restrict__ lds_top, uint32_t gl, float& best_t,
                                                int& best, uint32_t& c_nodes, uint32_t& c_leaves, uint32_t& c_tri,
                                                uint32_t& c_sph, uint32_t& c_replays, Coh& coh) {
  const WideView v = wide_view(a, r, lds_top);
  uint32_t sp = 0;
  const float4* q = v.top;
  WideNodeQ w;
  qnode_load(q, w);
  while (wide_iter_q<STATS, StackT>(
      a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves, c_tri, c_sph, coh)) {
  }
  wide_finish<STATS, StackT>(a, r, stk, gl, best_t, best, c_replays);
}

// The closest hit of a ray that can hit one sphere alone (render_loop ONE_SPHERE; DESIGN.md
// §3 "One-sphere tiles"): the reference reaches that sphere's test exactly when its leaf's
// box passes the loose test against t_max = +inf (§3 "Spheres"; static_ok on the planes in
// the ray's octant, as wide_iter's static_ok_slot applies it to a sphere slot), and with one
// candidate there is nothing to order.  Not for a degenerate ray (its octant is not defined).
__device__ __forceinline__ void one_sphere_hit(const KArgs& a, const RayT& r, float& best_t, int& best) {
  const OctSigns os(r);
  float entry;
  if (static_ok_planes(os.sx ? a.one_hi[0] : a.one_lo[0], os.sy ? a.one_hi[1] : a.one_lo[1],
                       os.sz ? a.one_hi[2] : a.one_lo[2], os.sx ? a.one_lo[0] : a.one_hi[0],
                       os.sy ? a.one_lo[1] : a.one_hi[1], os.sz ? a.one_lo[2] : a.one_hi[2], r, entry))
    sphere_test<false>(make_float4(a.one_rec[0], a.one_rec[1], a.one_rec[2], a.one_rec[3]), (int)a.one_slot, r, best_t,
                       best);
}

template <bool STATS, class StackT, bool PAXIS = false, bool LEAN = false>
__device__ __forceinline__ void traverse_wide(const KArgs& a, const RayT& r, StackT* __restrict__ stk,
                                              const float4* __restrict__ lds_top, uint32_t gl, float& best_t,
                                              int& best, uint32_t& c_nodes, uint32_t& c_leaves, uint32_t& c_tri,
                                              uint32_t& c_sph, uint32_t& c_replays, Coh& coh) {
  const WideView v = wide_view(a, r, lds_top);
  uint32_t sp = 0;
  // the root is node 0 of this octant's copy, in LDS with the other top levels
  const float4* q = v.top;
  WideNode w;
  const OctSigns os(r);
  wide_load(q, os.sx, os.sy, os.sz, w);
  while (wide_iter<STATS, StackT, true, PAXIS>(
      a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves, c_tri, c_sph, coh)) {
  }
  wide_finish<STATS, StackT, LEAN>(a, r, stk, gl, best_t, best, c_replays);
}

// ---------------------------------------------------------------------------
// shading
// ---------------------------------------------------------------------------
// @floatToInt(u64, f) then clamp(.., 0, n-1) as it executes on x86-64.
__device__ __forceinline__ uint32_t texel_index(float f, uint32_t n) {
  if (f >= 0.0f && f < 18446744073709551616.0f) {
    const float lim = (float)(n - 1);
    return f >= lim ? n - 1 : (uint32_t)f;
  }
  if (f < 0.0f && f > -1.0f) return 0;
  return n - 1;
}

// A material: the {u_off, v_off, kind, tex_kind} quad is read at the hit;
// color / image descriptor are read where the albedo is needed (keeping the
// whole 48-B record live across scatter spilled it to scratch).
struct MatReg {
  const float4* q;
  float4 m1;  // {u_off, v_off, kind, tex_kind}
  __device__ __forceinline__ uint32_t kind() const { return __float_as_uint(m1.z); }
  __device__ __forceinline__ uint32_t tex_kind() const { return __float_as_uint(m1.w); }
  __device__ __forceinline__ float ior() const { return q[0].w; }
};
__device__ __forceinline__ MatReg load_material(const DevMaterial* __restrict__ mats, uint32_t i) {
  const float4* q = reinterpret_cast<const float4*>(mats + i);
  return MatReg{q, q[1]};
}

// Attenuation codes.  What Material.scatter returns as the attenuation
// (material.zig:43-129) is one of: the (1,1,1) of a dielectric, a solid
// texture's color (a material's), or one texel of an image texture
// (texture.zig:20-74) - so a path stacks a 4-B code per scatter instead of
// three floats, and an image texel is fetched only when the product is taken
// (paths that end black never fetch theirs).  The values are the same f32s, so
// the product (att_product) is bit for bit the recursion's.
//   0xffffffff            dielectric (1, 1, 1)
//   1 << 31 | material    the material's solid color
//   1 << 30 | t           texel t of the f32 RGB store (a.texels)
//   t                     texel t of the 8-bit store (a.texels8, values k / 255)
// (t < 2^30: flatten_scene refuses larger stores)
constexpr uint32_t kAttOne = 0xffffffffu;

// texture.zig:20-74: the texel an image texture's albedo reads, as an att code
__device__ __forceinline__ uint32_t image_texel_code(const MatReg& mr, float u, float v) {
  const float4 m2 = mr.q[2];
  struct { float u_off, v_off; uint32_t img_w, img_h, img_off, img_u8; } m = {
      mr.m1.x, mr.m1.y, __float_as_uint(m2.x), __float_as_uint(m2.y), __float_as_uint(m2.z), __float_as_uint(m2.w)};
  const float uu_first = 1.0f - u + m.u_off;
  float uu = uu_first;
  if (uu_first > 1.0f) uu = uu_first - 1.0f;
  else if (uu_first < 0.0f) uu = uu_first + 1.0f;
  const float vv_first = v + m.v_off;
  float vv = vv_first;
  if (vv_first > 1.0f) vv = vv_first - 1.0f;
  else if (uu_first < 0.0f) vv = vv_first + 1.0f;  // texture.zig:66 tests uu_first
  const uint32_t x = texel_index(uu * (float)m.img_w, m.img_w);
  const uint32_t y = texel_index(vv * (float)m.img_h, m.img_h);
  const uint32_t t = m.img_off + y * m.img_w + x;  // < 2^30
  return m.img_u8 ? t : (1u << 30) | t;
}

// The albedo of a lambertian / metal hit (texture.zig:20-74) as an att code
template <bool LEAN = false>
__device__ __forceinline__ uint32_t albedo_code(const MatReg& mr, uint32_t mat, float u, float v) {
  if (Lean<LEAN>::tex || mr.tex_kind() == ZRT_TEX_COLOR) return (1u << 31) | mat;
  return image_texel_code(mr, u, v);
}

// The attenuation an att code stands for (the lean kernel's paths push one class
// of code only, a material's solid color)
template <bool LEAN = false>
__device__ __forceinline__ V3 att_value(const KArgs& a, const DevMaterial* __restrict__ mats, uint32_t code) {
  if (!Lean<LEAN>::diel && code == kAttOne) return mk(1.0f, 1.0f, 1.0f);
  if (Lean<LEAN>::tex || code >> 31) {
    const float4 c = reinterpret_cast<const float4*>(mats + (code & 0x7fffffffu))[0];
    return mk(c.x, c.y, c.z);
  }
  if (code >> 30) {
    const float* p = a.texels + 3ull * (code & 0x3fffffffu);
    return mk(p[0], p[1], p[2]);
  }
  // 4 B instead of 12 B per texel.  Its values are k / 255 (png_image.zig:88): the
  // correctly rounded quotient, which dev::div_known gives bit for bit for every
  // k in 0..255 (checked exactly: tests/test_host.py) - no dependent table loads
  const uint32_t px = a.texels8[code];
  constexpr float kInv255 = 1.0f / 255.0f;  // RN(1/255)
  return mk(dev::div_known(float(px & 0xffu), 255.0f, kInv255), dev::div_known(float((px >> 8) & 0xffu), 255.0f, kInv255),
            dev::div_known(float((px >> 16) & 0xffu), 255.0f, kInv255));
}

// raytrace.zig:53-58
// unit(d).y alone (vector.zig:88-92 for the one component backgroundColor reads)
__device__ __forceinline__ float unit_y(V3 v) {
  const float l = dev::sqrt_rn(v.x * v.x + v.y * v.y + v.z * v.z);
  if (__builtin_expect(ZRT_FAST_DIV && l >= 0x1p-50f && l <= 0x1p50f && __builtin_fabsf(v.y) >= l * 0x1p-50f, 1))
    return dev::div_core(v.y, l, dev::rcp_core(l));
  return v.y / l;
}

__device__ __forceinline__ V3 background(V3 d) {  // raytrace.zig:53-58
  const float t = 0.5f * (unit_y(d) + 1.0f);
  const float w = 1.0f - t;
  return mk(w + 0.5f * t, w + 0.7f * t, w + 1.0f * t);
}


// ---------------------------------------------------------------------------
// per-wave counter reduction: one 64-bit atomic per wave per counter
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wave_add_u64(unsigned long long* dst, uint32_t v) {
  uint32_t lo = v, hi = 0;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t olo = __shfl_xor(lo, off);
    const uint32_t ohi = __shfl_xor(hi, off);
    const uint32_t nlo = lo + olo;
    hi = hi + ohi + (nlo < lo ? 1u : 0u);
    lo = nlo;
  }
  if (__lane_id() == 0 && (lo | hi)) atomicAdd(dst, ((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void Coh::flush(unsigned long long* counters) {
  wave_add_u64(&counters[kGlobalNodes], gnodes);
  wave_add_u64(&counters[kUniformNodes], unodes);
  wave_add_u64(&counters[kPrimLaneTests], ptests);
  wave_add_u64(&counters[kUniformPrims], uprims);
  wave_add_u64(&counters[kAttWrites], attw);
  wave_add_u64(&counters[kAttReads], attr);
  wave_add_u64(&counters[kStackOvfWrites], ovfw);
  wave_add_u64(&counters[kVNodeTrips], vn_trips);
  wave_add_u64(&counters[kVNodeLines], vn_lines);
  wave_add_u64(&counters[kSNodeTrips], sn_trips);
  wave_add_u64(&counters[kRbTrips], rb_trips);
  wave_add_u64(&counters[kVPrimTrips], vp_trips);
  wave_add_u64(&counters[kVPrimLines], vp_lines);
  wave_add_u64(&counters[kSPrimTrips], sp_trips);
  wave_add_u64(&counters[kVShadeTrips], vsh_trips);
  wave_add_u64(&counters[kAttWTrips], attw_trips);
  wave_add_u64(&counters[kAttRTrips], attr_trips);
  wave_add_u64(&counters[kVNodeCost], vn_cost);
  wave_add_u64(&counters[kVPrimCost], vp_cost);
}

// ZRT_FLAG_SCANLINES: a finished unit's counters added to its frame rows.  The
// 8 lanes of a tile row (lanes 8k .. 8k+7) are summed with shuffles, then one
// lane per row adds them.  Called with the whole wave converged.
__device__ __forceinline__ void flush_scanline(unsigned long long* __restrict__ rows, uint32_t py, uint32_t height,
                                               int lane, uint32_t d, uint32_t r, uint32_t b) {
#pragma unroll
  for (int off = 1; off <= 4; off <<= 1) {
    d += __shfl_xor(d, off);
    r += __shfl_xor(r, off);
    b += __shfl_xor(b, off);
  }
  if ((lane & 7) == 0 && py < height) {
    if (d) atomicAdd(&rows[3 * py + 0], (unsigned long long)d);
    if (r) atomicAdd(&rows[3 * py + 1], (unsigned long long)r);
    if (b) atomicAdd(&rows[3 * py + 2], (unsigned long long)b);
  }
}

// ---------------------------------------------------------------------------
// the sampling loop
// ---------------------------------------------------------------------------
// LDS-typed pointers are 32-bit: a generic (flat) float* into LDS costs a 64-bit
// register pair across the whole loop (it was among the values the FAST kernel
// spilled to scratch)
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(3))) float lds_float;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
#else
typedef float lds_float;
typedef uint32_t lds_u32;
#endif
constexpr float kPi = 3.14159274101257324f;     // std.math.pi as f32
constexpr float kTwoPi = 6.28318548202514648f;  // comptime 2*pi as f32
constexpr float kInvPi = 1.0f / kPi;              // RN(1/pi), RN(1/(2pi)): dev::div_core's y
constexpr float kInvTwoPi = 1.0f / kTwoPi;

#ifndef ZRT_WAVES_PER_SIMD
#define ZRT_WAVES_PER_SIMD 8  // binary/reference; A/B (tools/ab.sh): w5 11.2, w6 12.1, w7 12.4, w8 12.6 Gray/s
#endif
#ifndef ZRT_WAVES_LIST
#define ZRT_WAVES_LIST 6      // list mode (C2); A/B: w5 27.8, w6 30.3, w8 28.7 Gray/s
#endif
#ifndef ZRT_WAVES_WIDE
#define ZRT_WAVES_WIDE 6      // FAST (wide tree) kernel, 80 VGPRs.  A/B, round 2 (96 VGPRs at w5): w4 46.0, w5 50.6,
                              // w6 48.2 (spills); round 4 (4-B att codes): C4 w5 52.5, w6 55.1, w7 44.8; C3 15.1 / 15.1 / 13.4
#endif

// The rest of one rayColor step after its closest-hit query (raytrace.zig:
// 71-100): a miss is the sky (backgroundColor); a hit is HitRecord.init
// (hit_record.zig:28-41) + Material.scatter (material.zig:43-129): absorbed
// ends the path black, a scatter pushes its attenuation (the product is taken
// in the recursion's order when the path ends) and moves the ray on.
// Where a path's attenuation rows (att codes) live: rows 0 .. a.att_lds_rows-1
// in LDS at lds[row * lds_stride], the rest in global memory at
// a.att[(row - a.att_lds_rows) * g_stride + g_index].  The lockstep, wavefront and
// list loops index them by lane (stride kBlock / a.n_lanes), the path-pool loop by path.
struct AttRows {
  lds_u32* __restrict__ lds;
  uint32_t lds_stride;
  uint64_t g_index;
  uint32_t g_stride;
};

// attenuation_1 * (attenuation_2 * (... * L)): the recursion's association
// (raytrace.zig:99), over the n rows a path pushed, read back in reverse
template <bool STATS>
__device__ __forceinline__ uint32_t att_row(const KArgs& a, const AttRows& ar, uint32_t i, Coh& coh) {
  if (i < a.att_lds_rows) return ar.lds[i * ar.lds_stride];
  if (STATS) {
    ++coh.attr;
    coh.attr_trips += wave_once();
  }
  const uint64_t k = (uint64_t)(i - a.att_lds_rows) * ar.g_stride + ar.g_index;
  return row_ok<STATS>(a, k, a.att_cap) ? a.att[k] : kAttOne;
}
template <bool STATS, bool LEAN = false>
__device__ __forceinline__ V3 att_product(const KArgs& a, const DevMaterial* __restrict__ mats, const AttRows& ar,
                                          uint32_t n, V3 col, Coh& coh) {
  uint32_t i = n;
  // two rows per trip: both texel loads are issued before either product, so a
  // textured path's chain of dependent fetches is half as long (the values and
  // the order of the multiplications are the recursion's, as below)
  for (; i >= 2; i -= 2) {
    const V3 hi = att_value<LEAN>(a, mats, att_row<STATS>(a, ar, i - 1, coh));
    const V3 lo = att_value<LEAN>(a, mats, att_row<STATS>(a, ar, i - 2, coh));
    col = mk(hi.x * col.x, hi.y * col.y, hi.z * col.z);
    col = mk(lo.x * col.x, lo.y * col.y, lo.z * col.z);
  }
  for (; i-- > 0;) {
    const V3 at = att_value<LEAN>(a, mats, att_row<STATS>(a, ar, i, coh));
    col = mk(at.x * col.x, at.y * col.y, at.z * col.z);
  }
  return col;
}

// HitRecord.init (hit_record.zig:28-41) of a closest hit: the material, the hit
// location, the normal flipped against the ray, and the texture coordinates
// (u, v) where the material reads an image.  shade_step's first half, and what
// features_kernel records of a first hit.
struct HitRec {
  MatReg mat;
  uint32_t tag, mkind;
  V3 loc, normal;
  float tu, tv;
  bool front;
};
template <bool STATS, bool LEAN>
__device__ __forceinline__ void hit_record(const KArgs& a, const DevMaterial* __restrict__ mats, int best,
                                           float best_t, const V3& o, const V3& d, uint32_t& c_shade,
                                           uint32_t& c_tex, Coh& coh, HitRec& h) {
  float4 sh;
  const int fb = __builtin_amdgcn_readfirstlane(best);
  if (__ballot(best != fb) == 0ull) {  // one hit surface in every lane here: scalar loads
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float4 cfloat4;
    sh = ((cfloat4*)a.shade)[fb];
#else
    sh = a.shade[fb];
#endif
  } else {
    if (STATS) coh.vsh_trips += wave_once();
    sh = a.shade[best];
  }
  const uint32_t tag = __float_as_uint(sh.w);
  const MatReg mat = load_material(mats, tag & 0x7fffffffu);
  const uint32_t mkind = mat.kind();
  const bool need_uv = !Lean<LEAN>::tex && mkind != ZRT_MAT_DIELECTRIC && mat.tex_kind() == ZRT_TEX_IMAGE;
  if (STATS) {
    ++c_shade;
    c_tex += need_uv ? 1u : 0u;
  }
  const V3 loc = add(o, scale(d, best_t));
  V3 outward;
  float tu = 0.0f, tv = 0.0f;
  if (tag >> 31) {
    outward = mk(sh.x, sh.y, sh.z);  // face_unit_normal
    if (need_uv) {  // barycentric (u, v), same arithmetic as the hit test
      const float4 p0 = a.prims[3 * best + 0];
      const float4 p1 = a.prims[3 * best + 1];
      const float4 p2 = a.prims[3 * best + 2];
      const V3 n = mk(p2.y, p2.z, p2.w);
      const float det = -dot(d, n);
      const float inv_det = inv_det_rn(det, a.tri_rcp_fast);
      const V3 ao = mk(o.x - p0.x, o.y - p0.y, o.z - p0.z);
      const V3 dao = cross(ao, d);
      tu = dot(mk(p1.z, p1.w, p2.x), dao) * inv_det;
      tv = -dot(mk(p0.w, p1.x, p1.y), dao) * inv_det;
    }
  } else {
    const float4 c = a.prims[3 * best];
    outward = scale(sub(loc, mk(c.x, c.y, c.z)), sh.x);  // (p - c) * (1/r)
    if (need_uv) {  // sphere.zig:47-51
      const float theta = dev::acos_z(-outward.y);
      const float phi = dev::atan2_z(-outward.z, -outward.x) + kPi;
      // phi in {+0} u [2^-23, 2pi], theta in {+0} u [2^-12, pi]: dev::div_core's
      // range, and +0 stays +0 (q = +0, r = +0, q + r*y = +0)
      tu = dev::div_known(phi, kTwoPi, kInvTwoPi);
      tv = dev::div_known(theta, kPi, kInvPi);
    }
  }
  bool front = true;
  V3 normal = outward;
  if (dot(d, outward) > 0.0f) {
    normal = neg(outward);
    front = false;
  }
  h.mat = mat;
  h.tag = tag;
  h.mkind = mkind;
  h.loc = loc;
  h.normal = normal;
  h.tu = tu;
  h.tv = tv;
  h.front = front;
}

template <bool STATS, class R, bool LEAN = false>
__device__ __forceinline__ void shade_step(const KArgs& a, const DevMaterial* __restrict__ mats,
                                           const AttRows& ar, R& rng, int best, float best_t,
                                           V3& o, V3& d, uint32_t& depth_left, bool& path_end, bool& sky, V3& L,
                                           uint32_t& c_bg, uint32_t& c_refl, uint32_t& c_shade, uint32_t& c_tex,
                                           Coh& coh) {
  if (best < 0) {
    ++c_bg;
    L = background(d);
    path_end = true;
    sky = true;
  } else {
    // ---- HitRecord.init (hit_record.zig:28-41)
    HitRec hr;
    hit_record<STATS, LEAN>(a, mats, best, best_t, o, d, c_shade, c_tex, coh, hr);
    const uint32_t tag = hr.tag;
    const MatReg mat = hr.mat;
    const uint32_t mkind = hr.mkind;
    const V3 loc = hr.loc;
    const V3 normal = hr.normal;
    const float tu = hr.tu, tv = hr.tv;
    const bool front = hr.front;
    // ---- Material.scatter (material.zig:43-129)
    bool absorbed = false;
    uint32_t att = kAttOne;  // the attenuation as an att code (dielectric: (1, 1, 1))
    V3 nd;
    if (mkind == ZRT_MAT_LAMBERTIAN) {
      const float r1 = rand_float(rng);
      const float r2 = rand_float(rng);
      const float rr = dev::sqrt_rn(1.0f - r1 * r1);
      float sn, cs;
      dev::sincos_z(kTwoPi * r2, &sn, &cs);
      V3 hv = mk(cs * rr, sn * rr, r1);
      if (!rand_bool(rng)) hv.z = hv.z * -1.0f;
      nd = unit(add(normal, hv));
      att = albedo_code<LEAN>(mat, tag & 0x7fffffffu, tu, tv);
    } else if (Lean<LEAN>::diel || mkind == ZRT_MAT_METAL) {  // (lean: what is not Lambertian is metal)
      nd = unit(reflect(unit(d), normal));
      if (dot(nd, normal) > 0.0f) att = albedo_code<LEAN>(mat, tag & 0x7fffffffu, tu, tv);
      else absorbed = true;
    } else {
      const float ratio = front ? dev::rcp_rn(mat.ior()) : mat.ior();
      const V3 ud = unit(d);
      const float cos_theta = dev::fmin_z(dot(neg(ud), normal), 1.0f);
      const float sin_theta = dev::sqrt_rn(1.0f - cos_theta * cos_theta);
      bool refl = ratio * sin_theta > 1.0f;
      if (!refl) {
        const float r0 = dev::div_rn(1.0f - ratio, 1.0f + ratio);
        const float reflectance = r0 + (1.0f - r0) * dev::pow5_z(1.0f - cos_theta);
        refl = reflectance > rand_float(rng);
      }
      nd = unit(refl ? reflect(ud, normal) : refract(ud, normal, ratio));
    }
    if (absorbed) {
      path_end = true;  // black
    } else {
      ++c_refl;
      if (depth_left > 1) {  // an attenuation pushed at depth 1 is never read
        // every earlier scatter was at a depth > this one, so all were pushed;
        // the first rows live in LDS, deeper ones in global memory
        const uint32_t i = a.max_depth - depth_left;
        if (i < a.att_lds_rows) {
          ar.lds[i * ar.lds_stride] = att;
        } else {
          const uint64_t k = (uint64_t)(i - a.att_lds_rows) * ar.g_stride + ar.g_index;
          if (row_ok<STATS>(a, k, a.att_cap)) a.att[k] = att;
          if (STATS) {
            ++coh.attw;
            coh.attw_trips += wave_once();
          }
        }
      }
      o = loc;
      d = nd;
      --depth_left;
    }
  }
}

// The lockstep loop's lane state parked in LDS across a traversal: the RNG
// state's words, then the chunk sums (r, g, b), the sample and the depth left,
// each a [word][lane] row of u32 (consecutive lanes, consecutive banks).  The
// traversal writes the stack rows of the same LDS, so the compiler cannot keep
// the values in registers past the traversal: they are stored and re-read.
template <int PRNG>
struct LaneState {
  static constexpr uint32_t kRngWords = sizeof(Rng<PRNG>) / 4;
  // (parking the ray's origin and direction too: 25 spills for 26, C4 -0.5 %, profiles/r06/r06c)
  static constexpr uint32_t kWords = kRngWords + 5;
  __device__ __forceinline__ static void park(lds_u32* p, const Rng<PRNG>& rng, float r, float g, float b,
                                              uint32_t sample, uint32_t depth) {
    uint32_t w[kRngWords];
    __builtin_memcpy(w, &rng, sizeof(w));
#pragma unroll
    for (uint32_t k = 0; k < kRngWords; ++k) p[k * kBlock] = w[k];
    p[(kRngWords + 0) * kBlock] = __float_as_uint(r);
    p[(kRngWords + 1) * kBlock] = __float_as_uint(g);
    p[(kRngWords + 2) * kBlock] = __float_as_uint(b);
    p[(kRngWords + 3) * kBlock] = sample;
    p[(kRngWords + 4) * kBlock] = depth;
  }
  __device__ __forceinline__ static void unpark(const lds_u32* p, Rng<PRNG>& rng, float& r, float& g, float& b,
                                                uint32_t& sample, uint32_t& depth) {
    uint32_t w[kRngWords];
#pragma unroll
    for (uint32_t k = 0; k < kRngWords; ++k) w[k] = p[k * kBlock];
    __builtin_memcpy(&rng, w, sizeof(w));
    r = __uint_as_float(p[(kRngWords + 0) * kBlock]);
    g = __uint_as_float(p[(kRngWords + 1) * kBlock]);
    b = __uint_as_float(p[(kRngWords + 2) * kBlock]);
    sample = p[(kRngWords + 3) * kBlock];
    depth = p[(kRngWords + 4) * kBlock];
  }
};

// The lockstep interval of a render launch after a scheduling probe (ZRT_AUTO_SYNC):
// the probe ran the same loop over every tile at one sample with the lanes in step,
// and its counters give the share of lane slots that ran a rayColor step (steps =
// reflections + sky hits + depth ends; absorbed metal paths, rare, are not counted).
// Where most lanes wait for a wave's longest path (the teapot, C3: 0.61 of the lane
// slots step, against 0.96 on the bunny, C4) the lanes run the unit's chunk freely
// instead of sample by sample: C3 +3.7 %, C4 -2.8 % with it (profiles/r05/r05l).
// Every wave reads the same counters, so every wave takes the same interval; the
// interval changes no result (each lane still renders its own samples in order).
#ifndef ZRT_AUTO_SYNC_UTIL
#define ZRT_AUTO_SYNC_UTIL 0.8  // lane-step share below which the lanes run free
#endif
__device__ __forceinline__ uint32_t auto_sync(const KArgs& a) {
  if (!a.sync_probe) return a.sync;
  const unsigned long long* p = a.sync_probe;
  const unsigned long long steps = p[kReflections] + p[kBackground] + p[kDepthHits];
  const unsigned long long slots = 64ull * p[kProbeTrips];
  return slots != 0 && double(steps) < ZRT_AUTO_SYNC_UTIL * double(slots) ? a.chunk : a.sync;
}

// StackT: uint16_t when the BVH has < 65536 nodes (halves the LDS stack, so
// more blocks fit per CU), uint32_t otherwise.
// PROBE: the scheduling probe's instance (schedule_probe_kernel): its one-sample
// units - one per tile, 65 536 on C4 - are dealt to the waves round-robin instead of
// through the global counter, whose one atomic per unit serialised the probe
// (the render launch's units are 32 samples and keep the counter)
// ONE_SPHERE: the instance for the tiles the host proved one-sphere (tile_class.cpp: no
// camera ray of theirs can return a hit from any primitive but the launch's one sphere,
// KArgs::one_*): a camera ray's step tests that sphere alone (one_sphere_hit) instead
// of walking the tree; every later step of the path is the loop's own.
template <int MODE /*0 list, 1 BVH binary, 2 BVH reference, 3 wide (FAST)*/, int PRNG, bool STATS, class StackT,
          bool PROBE = false, bool LEAN = false /* MODE 3, timed flavour: the lean kernel (struct Lean) */,
          bool ONE_SPHERE = false>
__device__ __forceinline__ void render_loop(const KArgs& a) {
  static_assert(!LEAN || (MODE == 3 && !STATS && !PROBE), "the lean kernel is the timed lockstep FAST loop's");
  static_assert(!ONE_SPHERE || (MODE == 3 && !PROBE), "the one-sphere step is the lockstep FAST loop's");
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;  // LDS: the traversal stack
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  lds_u32* att_l = (lds_u32*)(lds_raw + a.lds_att_off) + threadIdx.x;  // [row][lane] att codes
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const DevMaterial* mats = a.mats;
  // The lockstep loop reads the material table from its LDS copy only, through
  // LDS-typed pointers (ds_read), not a generic pointer chosen at run time (flat
  // loads); the host plans the table into LDS first and falls back to the wavefront
  // loop when it does not fit (C4 +1.5 %, C2 +0.5 %: profiles/r06/r06l).
  if (MODE == 3 || a.mats_in_lds) {  // (a.mats_in_lds: block-uniform)
    float4* m = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
    fill_lds_mats(a, m);
    mats = reinterpret_cast<const DevMaterial*>(m);
  }
  const int lane = (int)__lane_id();
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;  // n_lanes < 2^32
  // FAST: what a lane carries across its traversal - RNG state, chunk sums, sample,
  // depth - is parked in LDS ([word][lane], LaneState) while it traverses: the
  // traversal needs every VGPR of the 6-wave budget, and these values otherwise
  // went to scratch (9 stores + 9 loads per step through the vector-memory path)
  constexpr bool kLaneLds = MODE == 3;
  lds_u32* st_l = (lds_u32*)(lds_raw + a.lds_state_off) + threadIdx.x;

  bool active = false, in_sample = false;  // active: this lane still has samples in the wave's unit
  uint32_t sample = 0;
  // wave-uniform unit state (SGPRs): lanes run samples < gate; the unit (one
  // chunk of one tile) ends at unit_end; its tile lt has its corner at (x0, y0)
  uint32_t gate = 0, unit_end = 0, chunk_j = 0, x0 = 0, y0 = 0;
  uint32_t cur_lt = 0xffffffffu, iters = 0;  // the unit's tile, loop iterations spent on it
  const uint32_t sync = MODE == 3 ? auto_sync(a) : a.sync;  // lanes run samples < gate, `sync` at a time
  const uint64_t t_begin = ZRT_PROFILE ? __builtin_amdgcn_s_memrealtime() : 0;
  float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
  V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
  uint32_t depth_left = 0;  // attenuations stacked so far: max_depth - depth_left
  Rng<PRNG> rng;
  rng.init(0);
  uint32_t c_rays = 0, c_refl = 0, c_bg = 0, c_depth = 0, c_nodes = 0, c_tri = 0, c_sph = 0;
  uint32_t c_shade = 0, c_tex = 0, c_leaves = 0, c_replays = 0;
  Coh coh;  // STATS
  ExcessAcc excess;  // REFERENCE traversal, STATS flavour only

  uint64_t pf[5] = {0, 0, 0, 0, 0};  // refill, sample start, traversal, shading, path end
  // (PROBE: this wave's next unit; the waves of the grid take units w, w + W, w + 2W ..)
  uint32_t probe_u = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  uint32_t c_trips = 0, c_loops = 0, c_lsteps = 0, nodes_prev = 0;  // STATS: SIMD efficiency
  for (;;) {
    ++iters;
    if (STATS) {  // the wave is converged here: the previous step's traversal trips
      uint32_t m = c_nodes - nodes_prev;
      nodes_prev = c_nodes;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off));
      if (lane == 0) c_trips += m;
    }
    uint64_t t0 = prof_stamp();
    // ---- work: the WAVE takes units (local tile lt, a group of unit_chunks
    // chunks) from the global counter, one atomic per unit; lane p renders
    // pixel p of the unit's 8x8 tile.  The lanes run their paths on their own
    // but wait for each other every sync samples (gate), so the wave keeps
    // entering traversal and shading together and its camera rays stay
    // coherent: divergence, not memory, bounds this loop.
    const bool runnable = active && sample < gate;
    if (__ballot(runnable) == 0ull) {
      if (__ballot(active) != 0ull) {
        gate = min(gate + sync, unit_end);
      } else {
        if (cur_lt != 0xffffffffu)  // the finished unit's chunk sums, [chunk][pixel slot]: one 1 KiB store per wave
          a.partial[chunk_j * a.n_slots + cur_lt * 64u + (uint32_t)lane] = make_float4(acc_r, acc_g, acc_b, 0.0f);
        if (!Lean<LEAN>::epi && a.unit_cost && cur_lt != 0xffffffffu && lane == 0) {
          a.unit_cost[cur_lt] = iters;
          // (the probe's units are one sample: one of the unit's iterations ran no step)
          atomicAdd(&a.counters[kProbeTrips], (unsigned long long)(iters - 1u));
        }
        if (!Lean<LEAN>::epi && a.scanlines && cur_lt != 0xffffffffu) {  // the finished unit's counters, per frame row
          flush_scanline(a.scanlines, y0 + ((uint32_t)lane >> 3), a.height, lane, c_depth, c_refl, c_bg);
          c_depth = c_refl = c_bg = 0;  // (so the launch totals are the rows' sums)
        }
        uint32_t u = 0;
        if (PROBE) {
          u = probe_u;
          probe_u += gridDim.x * (kBlock / 64);
        } else {
          if (lane == 0) u = atomicAdd(a.work_counter, 1u);
          u = __builtin_amdgcn_readfirstlane(u);
        }
        if (u >= a.total_work) break;  // the counter is exhausted
        const uint32_t ord = u / a.n_chunks, g = u - ord * a.n_chunks;
        const uint32_t lt = a.tile_order ? a.tile_order[ord] : ord;  // costliest tiles first
        cur_lt = lt;
        iters = 0;
        const uint32_t t = lt * a.world + a.rank;  // local tile lt = global tile lt*world + rank
        x0 = (t % a.tiles_x) * 8u;
        y0 = (t / a.tiles_x) * 8u;
        chunk_j = g;
        sample = g * a.chunk;
        unit_end = min(sample + a.chunk, a.spp);
        gate = min(sample + sync, unit_end);
        // lane p renders pixel p of the 8x8 tile; off-frame lanes stay idle (finalize writes black)
        active = x0 + ((uint32_t)lane & 7u) < a.xbound && y0 + ((uint32_t)lane >> 3) < a.height;
        acc_r = acc_g = acc_b = 0.0f;
        in_sample = false;
      }
      if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[0] += t - t0; }
      continue;
    }
    if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[0] += t - t0; t0 = t; }
    if (STATS) {
      c_loops += lane == 0 ? 1u : 0u;
      c_lsteps += runnable ? 1u : 0u;
    }
    if (!runnable) continue;

    // ---- a new sample: jitter + Camera.getRay (raytrace.zig:173-175)
    if (!in_sample) {
      const uint32_t px = x0 + ((uint32_t)lane & 7u), py = y0 + ((uint32_t)lane >> 3);
      const uint64_t offset = (uint64_t)py * a.width + px;
      rng.init(((offset << 16) | (uint64_t)sample) + a.seed_mix);
      const float u = dev::div_known((float)px + rand_float(rng) - 0.5f, a.f_width, a.inv_width);
      const float v = dev::div_known((float)py + rand_float(rng) - 0.5f, a.f_height, a.inv_height);
      const V3 llc = mk(a.llc[0], a.llc[1], a.llc[2]);
      const V3 hor = mk(a.hor[0], a.hor[1], a.hor[2]);
      const V3 ver = mk(a.ver[0], a.ver[1], a.ver[2]);
      o = mk(a.org[0], a.org[1], a.org[2]);
      d = unit(sub(add(add(llc, scale(hor, u)), scale(ver, v)), o));
      depth_left = a.max_depth;
      in_sample = true;
    }
    if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[1] += t - t0; t0 = t; }

    // ---- one rayColor step (raytrace.zig:62-100)
    bool path_end = false, sky = false;
    V3 L = mk(0.0f, 0.0f, 0.0f);
    if (depth_left == 0) {
      ++c_depth;
      path_end = true;
    } else {
      if (STATS) ++c_rays;
      RayT r;
      r.ox = o.x; r.oy = o.y; r.oz = o.z;
      r.dx = d.x; r.dy = d.y; r.dz = d.z;
      r.rcp_det = a.tri_rcp_fast;
      r.gm = a.graze_m;
      r.gl = a.graze_leaf;
      r.gk = a.guard;
      inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
      float best_t = __builtin_inff();
      int best = -1;
      if (MODE == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
        // the list is wave-uniform: read it through the scalar cache (s_load)
        typedef const __attribute__((address_space(4))) float4 cfloat4;
        cfloat4* cprims = (cfloat4*)a.prims;
        cfloat4* cshade = (cfloat4*)a.shade;
#else
        const float4* cprims = a.prims;
        const float4* cshade = a.shade;
#endif
        for (uint32_t i = 0; i < a.n_list; ++i) {  // surfaces in list order, t_max shrinking
          const uint32_t tag = __float_as_uint(cshade[i].w);
          if (tag >> 31) {
            if (STATS) ++c_tri;
            tri_test_v<false>(cprims[3 * i], cprims[3 * i + 1], cprims[3 * i + 2], (int)i, r, best_t, best);
          } else {
            if (STATS) ++c_sph;
            sphere_test<false>(cprims[3 * i], (int)i, r, best_t, best);
          }
        }
      } else if (MODE == 3) {
        // (ONE_SPHERE: the camera ray, unless FAST would hand it to the replay - a rare lane-level branch)
        const bool walk = !ONE_SPHERE || depth_left != a.max_depth || ray_degenerate(r) ||
                          (!Lean<LEAN>::origin && !ray_origin_ok(a, r));
        if (walk) {
          if (kLaneLds) {
            LaneState<PRNG>::park(st_l, rng, acc_r, acc_g, acc_b, sample, depth_left);
          }
          traverse_wide<STATS, StackT, false, LEAN>(a, r, stk, lds_top, gl, best_t, best, c_nodes, c_leaves, c_tri, c_sph,
                                                    c_replays, coh);
          if (kLaneLds) {
            LaneState<PRNG>::unpark(st_l, rng, acc_r, acc_g, acc_b, sample, depth_left);
          }
        } else {
          if (STATS) ++c_sph;  // (per short-path ray, whether or not the leaf box lets the test run)
          one_sphere_hit(a, r, best_t, best);
        }
      } else {
        traverse_bvh<MODE == 1, STATS>(a, r, stk, best_t, best, c_nodes, c_tri, c_sph, &excess);
      }
      if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[2] += t - t0; t0 = t; }
      shade_step<STATS, Rng<PRNG>, LEAN>(a, mats, AttRows{att_l, kBlock, gl, a.n_lanes}, rng, best, best_t, o, d, depth_left,
                                         path_end, sky, L, c_bg, c_refl, c_shade, c_tex, coh);
    }

    if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[3] += t - t0; t0 = t; }
    if (path_end) {
      // a path that reached the sky traced at depth_left >= 1: all of its
      // max_depth - depth_left scatters were pushed
      const V3 col = sky ? att_product<STATS, LEAN>(a, mats, AttRows{att_l, kBlock, gl, a.n_lanes}, a.max_depth - depth_left, L, coh) : L;
      acc_r += col.x;
      acc_g += col.y;
      acc_b += col.z;
      in_sample = false;
      if (++sample == unit_end) active = false;  // chunk done: its sequential sum, stored when the unit ends
    }
    if (ZRT_PROFILE) { const uint64_t t = prof_stamp(); pf[4] += t - t0; }
  }
  if (ZRT_PROFILE && lane == 0) {
    for (int k = 0; k < 5; ++k) atomicAdd(&a.counters[kProfSlot + k], (unsigned long long)pf[k]);
    if (a.wave_times) {
      const uint32_t w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
      a.wave_times[2 * w] = t_begin;
      a.wave_times[2 * w + 1] = __builtin_amdgcn_s_memrealtime();
    }
  }

  wave_add_u64(&a.counters[kDepthHits], c_depth);
  wave_add_u64(&a.counters[kReflections], c_refl);
  wave_add_u64(&a.counters[kBackground], c_bg);
  if (STATS) {
    wave_add_u64(&a.counters[kRays], c_rays);
    wave_add_u64(&a.counters[kNodes], c_nodes);
    wave_add_u64(&a.counters[kTriTests], c_tri);
    wave_add_u64(&a.counters[kSphereTests], c_sph);
    wave_add_u64(&a.counters[kShades], c_shade);
    wave_add_u64(&a.counters[kTexels], c_tex);
    wave_add_u64(&a.counters[kLeaves], c_leaves);
    wave_add_u64(&a.counters[kReplays], c_replays);
    wave_add_u64(&a.counters[kTravTrips], c_trips);
    wave_add_u64(&a.counters[kLoopTrips], c_loops);
    wave_add_u64(&a.counters[kLaneSteps], c_lsteps);
    coh.flush(a.counters);
    if (MODE == 2) {
      // maxima of non-negative floats: their bit patterns order like unsigned ints
      uint32_t mt = __float_as_uint(excess.tri), ms = __float_as_uint(excess.sph);
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        mt = max(mt, (uint32_t)__shfl_xor((int)mt, off));
        ms = max(ms, (uint32_t)__shfl_xor((int)ms, off));
      }
      if (lane == 0) {
        atomicMax(&a.counters[kExcessTri], (unsigned long long)mt);
        atomicMax(&a.counters[kExcessSph], (unsigned long long)ms);
      }
      wave_add_u64(&a.counters[kExcessHits], excess.over);
    }
  }
}

// ---------------------------------------------------------------------------
// The wavefront loop (FAST traversal, MODE 4).  render_loop keeps a wave's 64
// lanes in lockstep: every lane traces one ray per loop step and the wave
// waits for its slowest traversal.  Where traversal lengths vary a lot between
// lanes (a large mesh filling the frame: teapot, C5) most lanes idle most of
// the time (tools/simd_eff.py: 22-29 % traversal lane efficiency on C3/C5 vs
// 74 % on the bunny).  Here a lane's traversal is suspended between nodes
// (wide_iter), and the wave alternates two phases, chosen with __ballot:
//   traverse: node steps for the lanes with a ray in flight, until at least
//             wf_thresh/64 of the unit's active lanes have finished theirs
//             (the others stay suspended: node, stack, best hit kept);
//   shade:    the finished lanes, together, run the rest of their rayColor
//             step (shade_step) and set up their next ray - the scattered one,
//             or the camera ray of their pixel's next sample - so they rejoin
//             the traversal while the suspended lanes go on.
// The active-ray set is compacted by the ballot counts (no lane waits for the
// whole wave's traversal), the stacks stay in LDS per lane, and every lane
// still renders its own pixel's samples in order (sequential chunk sums, the
// attenuation stack in the recursion's order): images are bit-identical to
// render_loop's.
// ---------------------------------------------------------------------------
template <int PRNG, bool STATS, class StackT>
__device__ __forceinline__ void render_loop_wf(const KArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;  // LDS: the traversal stack
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  lds_u32* att_l = (lds_u32*)(lds_raw + a.lds_att_off) + threadIdx.x;  // [row][lane] att codes
  if (!layout_ok(a)) return;
  fill_lds_top(a, lds_top);
  const DevMaterial* mats = a.mats;
  if (a.mats_in_lds) {  // block-uniform
    float4* m = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
    fill_lds_mats(a, m);
    mats = reinterpret_cast<const DevMaterial*>(m);
  }
  const int lane = (int)__lane_id();
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;

  bool active = false;     // this lane has samples left in the wave's unit
  bool in_sample = false;  // ... and one of them is under way
  bool trav = false;       // ... whose current ray is being traversed
  uint32_t sample = 0;
  uint32_t unit_end = 0, chunk_j = 0, x0 = 0, y0 = 0, cur_lt = 0xffffffffu;  // wave-uniform
  float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
  V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
  uint32_t depth_left = 0;
  Rng<PRNG> rng;
  rng.init(0);
  // the ray in flight and its suspended traversal
  RayT r{};
  r.rcp_det = a.tri_rcp_fast;
  r.gm = a.graze_m;
  r.gl = a.graze_leaf;
  r.gk = a.guard;
  float best_t = __builtin_inff();
  int best = -1;
  uint32_t sp = 0;
  const float4* q = nullptr;  // the lane's current node (LDS or global)
  uint32_t c_rays = 0, c_refl = 0, c_bg = 0, c_depth = 0, c_nodes = 0, c_tri = 0, c_sph = 0;
  uint32_t c_shade = 0, c_tex = 0, c_leaves = 0, c_replays = 0;
  Coh coh;  // STATS
  uint32_t c_trips = 0, c_loops = 0, c_lsteps = 0;  // STATS: SIMD efficiency

  for (;;) {
    // ---- traverse: node steps while enough lanes still have a ray in flight
    {
      const uint32_t n_act = (uint32_t)__builtin_popcountll(__ballot(active));
      const uint32_t thresh = max(1u, (n_act * a.wf_thresh) >> 6);
      WideView v{};
      WideNode w;
      if (trav) {
        v = wide_view(a, r, lds_top);
        const OctSigns os(r);
        wide_load(q, os.sx, os.sy, os.sz, w);  // the suspended node (re)loaded
      }
      for (;;) {
        if (trav) {
          // (its lanes' nodes are rarely one: no scalar-load test, C5 -1.4 % with it)
          if (!wide_iter<STATS, StackT, false, true, false>(a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves, c_tri,
                                               c_sph, coh)) {
            wide_finish<STATS, StackT>(a, r, stk, gl, best_t, best, c_replays);
            trav = false;
          }
        }
        if (STATS) c_trips += lane == 0 ? 1u : 0u;
        if (__ballot(trav) == 0ull) break;
        if ((uint32_t)__builtin_popcountll(__ballot(active && !trav)) >= thresh) break;
      }
    }
    // ---- refill: the wave's unit is done (lanes wait at unit ends only)
    if (__ballot(active) == 0ull) {
      // the finished unit's chunk sums, [chunk][pixel slot], all 64 lanes at once: one
      // 1 KiB store per wave (stored by each lane as it finished, the lines went out
      // to memory in 32-B pieces: twice the bytes, profiles/r03 write budget)
      if (cur_lt != 0xffffffffu)
        a.partial[chunk_j * a.n_slots + cur_lt * 64u + (uint32_t)lane] = make_float4(acc_r, acc_g, acc_b, 0.0f);
      if (a.scanlines && cur_lt != 0xffffffffu) {
        flush_scanline(a.scanlines, y0 + ((uint32_t)lane >> 3), a.height, lane, c_depth, c_refl, c_bg);
        c_depth = c_refl = c_bg = 0;
      }
      uint32_t u = 0;
      if (lane == 0) u = atomicAdd(a.work_counter, 1u);
      u = __builtin_amdgcn_readfirstlane(u);
      if (u >= a.total_work) break;  // the counter is exhausted
      const uint32_t ord = u / a.n_chunks, g = u - ord * a.n_chunks;
      const uint32_t lt = a.tile_order ? a.tile_order[ord] : ord;  // costliest tiles first
      cur_lt = lt;
      const uint32_t t = lt * a.world + a.rank;
      x0 = (t % a.tiles_x) * 8u;
      y0 = (t / a.tiles_x) * 8u;
      chunk_j = g;
      sample = g * a.chunk;
      unit_end = min(sample + a.chunk, a.spp);
      active = x0 + ((uint32_t)lane & 7u) < a.xbound && y0 + ((uint32_t)lane >> 3) < a.height;
      acc_r = acc_g = acc_b = 0.0f;
      in_sample = false;
      trav = false;
    }
    // ---- shade: the lanes whose ray is done, together
    if (STATS) {
      c_loops += lane == 0 ? 1u : 0u;
      c_lsteps += active && !trav ? 1u : 0u;
    }
    if (!active || trav) continue;
    bool path_end = false, sky = false;
    V3 L = mk(0.0f, 0.0f, 0.0f);
    if (in_sample) {
      shade_step<STATS>(a, mats, AttRows{att_l, kBlock, gl, a.n_lanes}, rng, best, best_t, o, d, depth_left, path_end,
                        sky, L, c_bg, c_refl, c_shade, c_tex, coh);
      if (!path_end && depth_left == 0) {  // the next rayColor is at depth 0: black (raytrace.zig:64-67)
        ++c_depth;
        path_end = true;
      }
    }
    if (path_end) {
      const V3 col = sky ? att_product<STATS>(a, mats, AttRows{att_l, kBlock, gl, a.n_lanes}, a.max_depth - depth_left, L, coh) : L;
      acc_r += col.x;
      acc_g += col.y;
      acc_b += col.z;
      in_sample = false;
      if (++sample == unit_end) {  // chunk done: its sequential sum (stored at the unit's end)
        active = false;
        continue;
      }
    }
    if (!in_sample) {  // a new sample: jitter + Camera.getRay (raytrace.zig:173-175); max_depth >= 1 here
      const uint32_t px = x0 + ((uint32_t)lane & 7u), py = y0 + ((uint32_t)lane >> 3);
      const uint64_t offset = (uint64_t)py * a.width + px;
      rng.init(((offset << 16) | (uint64_t)sample) + a.seed_mix);
      const float u = dev::div_known((float)px + rand_float(rng) - 0.5f, a.f_width, a.inv_width);
      const float vv = dev::div_known((float)py + rand_float(rng) - 0.5f, a.f_height, a.inv_height);
      const V3 llc = mk(a.llc[0], a.llc[1], a.llc[2]);
      const V3 hor = mk(a.hor[0], a.hor[1], a.hor[2]);
      const V3 ver = mk(a.ver[0], a.ver[1], a.ver[2]);
      o = mk(a.org[0], a.org[1], a.org[2]);
      d = unit(sub(add(add(llc, scale(hor, u)), scale(ver, vv)), o));
      depth_left = a.max_depth;
      in_sample = true;
    }
    // ---- the next closest-hit query (raytrace.zig:71-81): suspended at the root
    if (STATS) ++c_rays;
    r.ox = o.x; r.oy = o.y; r.oz = o.z;
    r.dx = d.x; r.dy = d.y; r.dz = d.z;
    inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
        best_t = __builtin_inff();
    best = -1;
    sp = 0;
    {
      const WideView v = wide_view(a, r, lds_top);
      q = v.top;
    }
    trav = true;
  }

  wave_add_u64(&a.counters[kDepthHits], c_depth);
  wave_add_u64(&a.counters[kReflections], c_refl);
  wave_add_u64(&a.counters[kBackground], c_bg);
  if (STATS) {
    wave_add_u64(&a.counters[kRays], c_rays);
    wave_add_u64(&a.counters[kNodes], c_nodes);
    wave_add_u64(&a.counters[kTriTests], c_tri);
    wave_add_u64(&a.counters[kSphereTests], c_sph);
    wave_add_u64(&a.counters[kShades], c_shade);
    wave_add_u64(&a.counters[kTexels], c_tex);
    wave_add_u64(&a.counters[kLeaves], c_leaves);
    wave_add_u64(&a.counters[kReplays], c_replays);
    wave_add_u64(&a.counters[kTravTrips], c_trips);
    wave_add_u64(&a.counters[kLoopTrips], c_loops);
    wave_add_u64(&a.counters[kLaneSteps], c_lsteps);
    coh.flush(a.counters);
  }
}

// ---------------------------------------------------------------------------
// The path-pool loop (FAST traversal, MODE 5): the wavefront loop with its rays
// decoupled from lanes.  A wave holds two 64-pixel units at a time (unit slots
// 0 and 1) - 128 paths, each one pixel's current sample - and a queue of the
// paths whose next ray waits for traversal, in LDS.  Two phases alternate,
// chosen with __ballot:
//   traverse: every lane without a ray takes the next queued one - lane k of
//             the idle lanes (mbcnt rank over the ballot of idle lanes) takes
//             queue entry head + k, so the queue is compacted onto the idle
//             lanes - and takes node steps; a finished traversal writes its
//             hit to the path's LDS record and the lane takes the next ray.
//             The phase ends when the queue is empty and fewer than
//             wf_thresh / 64 of the lanes still traverse (the others stay
//             suspended: node, stack, best hit kept in registers).
//   shade:    lane q owns paths q and 64 + q (pixel q of each unit) and shades
//             those whose hit is in (shade_step): the scattered ray, or its
//             pixel's next camera ray, is appended to the queue (ballot +
//             mbcnt again); a unit whose 64 paths have finished their chunk
//             stores its chunk sums and takes the next unit from the global
//             counter.
// A pixel's samples still run one after another on one path, summed in order
// by its owner lane, and every path's attenuations are stacked per path in the
// recursion's order: images are bit-identical to render_loop's.  Rays move
// between lanes, traversals never do (a lane keeps its ray, stack column and
// node until the traversal ends).
// ---------------------------------------------------------------------------
constexpr uint32_t kPoolPaths = 128;                           // per wave: two unit slots of 64 paths
constexpr uint32_t kBlockPaths = kPoolPaths * (kBlock / 64);   // per block
constexpr int32_t kHitPending = -2;                            // a path's hit record before its traversal ends

// One path's state, held by its owner lane: its pixel's sample under way (a path
// whose sample reached its unit's end is done) and the depth left, packed
// (both u16: RenderParams, raytrace.zig:102-108), the chunk's running sum.
template <int PRNG>
struct PathReg {
  Rng<PRNG> rng;
  uint32_t ds;  // depth_left << 16 | sample
  float acc_r, acc_g, acc_b;
  __device__ __forceinline__ uint32_t sample() const { return ds & 0xffffu; }
  __device__ __forceinline__ uint32_t depth_left() const { return ds >> 16; }
};

// ZRT_FLAG_SCANLINES: a path's counter events go straight to its frame row
// (paths of one unit finish at different times here); raytrace.zig:184
__device__ __forceinline__ void scanline_add(const KArgs& a, uint32_t py, uint32_t k, uint32_t n) {
  if (n != 0u && py < a.height) atomicAdd(&a.scanlines[3 * py + k], (unsigned long long)n);
}

// The pool's LDS: rays [6][kBlockPaths] (o.xyz, d.xyz), hits t / slot
// [kBlockPaths], the per-wave queues [waves][kPoolPaths] of path ids.
struct PoolLds {
  lds_float* ray;
  lds_float* hit_t;
  __attribute__((address_space(3))) int32_t* hit_p;
  __attribute__((address_space(3))) uint8_t* queue;  // this wave's
};

// Where a path's attenuation rows past LDS go: [path][row] keeps one path's rows in
// one or two 32-B sectors, so its pushes of one sample (and the next samples') merge
// in L2 before they are written back; [row][path] would spread them, every 4-B code a
// sector of its own (the pool's lanes shade paths at unrelated depths).
template <int PRNG, bool STATS, class StackT, bool GUARD, bool QN = false>
__device__ __forceinline__ void render_loop_pool(const KArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;  // LDS: the lane's traversal stack column
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if (!layout_ok(a)) return;
  fill_lds_top(a, lds_top);
  const DevMaterial* mats = a.mats;
  if (a.mats_in_lds) {  // block-uniform
    float4* m = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
    fill_lds_mats(a, m);
    mats = reinterpret_cast<const DevMaterial*>(m);
  }
  const int lane = (int)__lane_id();
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t wave_paths = (threadIdx.x >> 6) * kPoolPaths;  // this wave's first path in the block
  const uint64_t g_paths = (uint64_t)blockIdx.x * kBlockPaths;  // the block's first path in the launch
  PoolLds pl;
  {
    lds_float* base = (lds_float*)(lds_raw + a.lds_pool_off);
    pl.ray = base;
    pl.hit_t = base + 6 * kBlockPaths;
    pl.hit_p = (__attribute__((address_space(3))) int32_t*)(base + 7 * kBlockPaths);
    pl.queue = (__attribute__((address_space(3))) uint8_t*)(base + 8 * kBlockPaths) + wave_paths;
  }
  lds_u32* att_base = (lds_u32*)(lds_raw + a.lds_att_off);  // [row][path of the block] att codes
  // global rows past the LDS ones: [path][row], g_rows per path
  const uint32_t g_rows = a.max_depth > a.att_lds_rows ? a.max_depth - a.att_lds_rows : 1u;

  // unit slots (wave-uniform): tile, chunk, the samples [.., unit_end) of the chunk
  bool slot_on[2] = {false, false};
  uint32_t s_lt[2] = {0xffffffffu, 0xffffffffu}, s_chunk[2] = {0, 0}, s_end[2] = {0, 0}, s_x0[2] = {0, 0},
           s_y0[2] = {0, 0};
  bool exhausted = false;  // the global unit counter ran out
  PathReg<PRNG> pA, pB;    // paths lane and 64 + lane (done: sample >= the slot's unit end, 0 while it is off)
  pA.acc_r = pA.acc_g = pA.acc_b = pB.acc_r = pB.acc_g = pB.acc_b = 0.0f;
  pA.ds = pB.ds = 0;
  pA.rng.init(0);
  pB.rng.init(0);
  uint32_t c_depth = 0, c_refl = 0, c_bg = 0;  // Progress counters (raytrace.zig:20-34) of this lane's paths
  uint32_t q_head = 0, q_tail = 0;  // wave-uniform queue positions (mod kPoolPaths)

  // the ray in flight on this lane and its suspended traversal
  bool trav = false;
  uint32_t cp = 0;  // its path (0 .. kPoolPaths-1 of this wave)
  RayT r{};
  r.rcp_det = a.tri_rcp_fast;
  r.gm = a.graze_m;
  r.gl = a.graze_leaf;
  r.gk = GUARD ? a.guard : 0.0f;
  float best_t = __builtin_inff();
  int best = -1;
  uint32_t sp = 0;
  const float4* q = nullptr;
  uint32_t c_rays = 0, c_nodes = 0, c_tri = 0, c_sph = 0, c_shade = 0, c_tex = 0, c_leaves = 0, c_replays = 0;
  Coh coh;  // STATS
  uint32_t c_trips = 0, c_loops = 0, c_lsteps = 0;

  for (;;) {
    // ---- traverse: idle lanes take queued rays; node steps
    {
      // shade once the queue is empty and fewer than 64 - wf_thresh lanes still traverse
      const uint32_t thresh = 64u - a.wf_thresh;
      WideView v{};
      std::conditional_t<QN, WideNodeQ, WideNode> w;
      if (trav) {
        v = wide_view(a, r, lds_top);
        node_load<QN>(q, r, w);  // the suspended node (re)loaded
      }
      for (;;) {
        const uint64_t idle = __ballot(!trav);
        const uint32_t avail = q_tail - q_head;
        if (idle != 0ull && avail != 0u) {
          const uint32_t rank = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(idle >> 32),
                                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)idle, 0u));
          if (!trav && rank < avail) {  // the rank-th idle lane takes queue entry head + rank
            cp = pl.queue[(q_head + rank) & (kPoolPaths - 1u)];
            const uint32_t P = wave_paths + cp;
            const V3 o = mk(pl.ray[0 * kBlockPaths + P], pl.ray[1 * kBlockPaths + P], pl.ray[2 * kBlockPaths + P]);
            const V3 d = mk(pl.ray[3 * kBlockPaths + P], pl.ray[4 * kBlockPaths + P], pl.ray[5 * kBlockPaths + P]);
            if (STATS) ++c_rays;
            r.ox = o.x; r.oy = o.y; r.oz = o.z;
            r.dx = d.x; r.dy = d.y; r.dz = d.z;
            inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
            best_t = __builtin_inff();
            best = -1;
            sp = 0;
            v = wide_view(a, r, lds_top);
            q = v.top;
            node_load<QN>(q, r, w);
            trav = true;
          }
          const uint32_t n_idle = (uint32_t)__builtin_popcountll(idle);
          q_head += n_idle < avail ? n_idle : avail;
        }
        if (trav) {
          bool more;
          if constexpr (QN)
            more = wide_iter_q<STATS, StackT, true, GUARD>(a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves,
                                                          c_tri, c_sph, coh);
          else
            more = wide_iter<STATS, StackT, false, true, GUARD>(a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves,
                                                                c_tri, c_sph, coh);
          if (!more) {
            wide_finish<STATS, StackT>(a, r, stk, gl, best_t, best, c_replays);
            const uint32_t P = wave_paths + cp;
            pl.hit_t[P] = best_t;
            pl.hit_p[P] = best;
            trav = false;
          }
        }
        if (STATS) c_trips += lane == 0 ? 1u : 0u;
        const uint32_t n_trav = (uint32_t)__builtin_popcountll(__ballot(trav));
        if (n_trav == 0u) break;
        if (q_tail == q_head && n_trav < thresh) break;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // hits written by other lanes of the wave
    // ---- shade: owners shade their paths whose hit is in; units end and refill
#pragma unroll 1
    for (uint32_t s = 0; s < 2; ++s) {
      const uint32_t p = s * 64u + (uint32_t)lane, P = wave_paths + p;
      const AttRows ar{att_base + P, kBlockPaths, (g_paths + P) * g_rows, 1u};
      const uint32_t unit_end = s ? s_end[1] : s_end[0];
      const uint32_t x0 = s ? s_x0[1] : s_x0[0], y0 = s ? s_y0[1] : s_y0[0];
      bool push = false;
      const uint32_t py = y0 + ((uint32_t)lane >> 3);
      if (pA.sample() < unit_end && pl.hit_p[P] != kHitPending) {
        if (STATS) {
          c_lsteps += 1u;
        }
        V3 o = mk(pl.ray[0 * kBlockPaths + P], pl.ray[1 * kBlockPaths + P], pl.ray[2 * kBlockPaths + P]);
        V3 d = mk(pl.ray[3 * kBlockPaths + P], pl.ray[4 * kBlockPaths + P], pl.ray[5 * kBlockPaths + P]);
        const int hb = pl.hit_p[P];
        const float ht = pl.hit_t[P];
        bool path_end = false, sky = false;
        V3 L = mk(0.0f, 0.0f, 0.0f);
        uint32_t dl = pA.depth_left();
        const uint32_t bg0 = c_bg, rf0 = c_refl;
        shade_step<STATS>(a, mats, ar, pA.rng, hb, ht, o, d, dl, path_end, sky, L, c_bg, c_refl, c_shade, c_tex, coh);
        uint32_t dh = 0;
        if (!path_end && dl == 0) {  // the next rayColor is at depth 0: black (raytrace.zig:64-67)
          ++c_depth;
          dh = 1;
          path_end = true;
        }
        if (a.scanlines) {
          scanline_add(a, py, 0, dh);
          scanline_add(a, py, 1, c_refl - rf0);
          scanline_add(a, py, 2, c_bg - bg0);
        }
        uint32_t smp = pA.sample();
        if (path_end) {
          const V3 col = sky ? att_product<STATS>(a, mats, ar, a.max_depth - dl, L, coh) : L;
          pA.acc_r += col.x;
          pA.acc_g += col.y;
          pA.acc_b += col.z;
          if (++smp < unit_end) {  // the pixel's next sample: jitter + Camera.getRay (raytrace.zig:173-175)
            // (at the unit's end the path is done: its chunk's sequential sum is stored with the unit)
            const uint32_t px = x0 + ((uint32_t)lane & 7u);
            pA.rng.init((((uint64_t)py * a.width + px) << 16 | (uint64_t)smp) + a.seed_mix);
            const float u = dev::div_known((float)px + rand_float(pA.rng) - 0.5f, a.f_width, a.inv_width);
            const float vv = dev::div_known((float)py + rand_float(pA.rng) - 0.5f, a.f_height, a.inv_height);
            o = mk(a.org[0], a.org[1], a.org[2]);
            d = unit(sub(add(add(mk(a.llc[0], a.llc[1], a.llc[2]), scale(mk(a.hor[0], a.hor[1], a.hor[2]), u)),
                             scale(mk(a.ver[0], a.ver[1], a.ver[2]), vv)),
                         o));
            dl = a.max_depth;
            push = true;
          }
        } else {
          push = true;  // the scattered ray
        }
        pA.ds = dl << 16 | smp;
        if (push) {
          pl.ray[0 * kBlockPaths + P] = o.x; pl.ray[1 * kBlockPaths + P] = o.y; pl.ray[2 * kBlockPaths + P] = o.z;
          pl.ray[3 * kBlockPaths + P] = d.x; pl.ray[4 * kBlockPaths + P] = d.y; pl.ray[5 * kBlockPaths + P] = d.z;
          pl.hit_p[P] = kHitPending;
        }
      }
      // the unit in slot s is over: its chunk sums (one 1 KiB store), its rows' counters; the next unit
      const bool s_on = s ? slot_on[1] : slot_on[0];
      if (__ballot(pA.sample() < unit_end) == 0ull && (s_on || !exhausted)) {
        const uint32_t lt = s ? s_lt[1] : s_lt[0];
        if (s_on) {
          const uint32_t cj = s ? s_chunk[1] : s_chunk[0];
          a.partial[cj * a.n_slots + lt * 64u + (uint32_t)lane] = make_float4(pA.acc_r, pA.acc_g, pA.acc_b, 0.0f);
        }
        uint32_t u = a.total_work;
        if (!exhausted) {
          if (lane == 0) u = atomicAdd(a.work_counter, 1u);
          u = __builtin_amdgcn_readfirstlane(u);
        }
        bool on = false;
        uint32_t nlt = 0xffffffffu, g = 0, nx0 = 0, ny0 = 0;
        if (u < a.total_work) {
          const uint32_t ord = u / a.n_chunks;
          g = u - ord * a.n_chunks;
          nlt = a.tile_order ? a.tile_order[ord] : ord;  // costliest tiles first
          const uint32_t t = nlt * a.world + a.rank;
          nx0 = (t % a.tiles_x) * 8u;
          ny0 = (t / a.tiles_x) * 8u;
          on = true;
        } else {
          exhausted = true;
        }
        if (s) { slot_on[1] = on; s_lt[1] = nlt; s_chunk[1] = g; s_x0[1] = nx0; s_y0[1] = ny0; }
        else { slot_on[0] = on; s_lt[0] = nlt; s_chunk[0] = g; s_x0[0] = nx0; s_y0[0] = ny0; }
        pA.acc_r = pA.acc_g = pA.acc_b = 0.0f;
        const uint32_t first = g * a.chunk, end = on ? min(first + a.chunk, a.spp) : 0u;
        if (s) s_end[1] = end;
        else s_end[0] = end;
        pA.ds = end;  // done, unless its pixel is on the frame
        if (on) {
          const uint32_t px = nx0 + ((uint32_t)lane & 7u), ny = ny0 + ((uint32_t)lane >> 3);
          // pixel q of the tile; off-frame paths stay done (finalize writes black)
          if (px < a.xbound && ny < a.height) {
            pA.rng.init((((uint64_t)ny * a.width + px) << 16 | (uint64_t)first) + a.seed_mix);
            const float uu = dev::div_known((float)px + rand_float(pA.rng) - 0.5f, a.f_width, a.inv_width);
            const float vv = dev::div_known((float)ny + rand_float(pA.rng) - 0.5f, a.f_height, a.inv_height);
            const V3 o = mk(a.org[0], a.org[1], a.org[2]);
            const V3 d = unit(sub(add(add(mk(a.llc[0], a.llc[1], a.llc[2]), scale(mk(a.hor[0], a.hor[1], a.hor[2]), uu)),
                                      scale(mk(a.ver[0], a.ver[1], a.ver[2]), vv)),
                                  o));
            pA.ds = a.max_depth << 16 | first;
            pl.ray[0 * kBlockPaths + P] = o.x; pl.ray[1 * kBlockPaths + P] = o.y; pl.ray[2 * kBlockPaths + P] = o.z;
            pl.ray[3 * kBlockPaths + P] = d.x; pl.ray[4 * kBlockPaths + P] = d.y; pl.ray[5 * kBlockPaths + P] = d.z;
            pl.hit_p[P] = kHitPending;
            push = true;
          }
        }
      }
      // append the new rays to the queue: the rank-th pushing lane at tail + rank
      const uint64_t pm = __ballot(push);
      if (pm != 0ull) {
        const uint32_t rank = (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32),
                                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0u));
        if (push) pl.queue[(q_tail + rank) & (kPoolPaths - 1u)] = (uint8_t)p;
        q_tail += (uint32_t)__builtin_popcountll(pm);
      }
      // the other path's state to the front (both slots go through the same code)
      { PathReg<PRNG> t = pA; pA = pB; pB = t; }
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // rays and queue entries written by other lanes
    if (STATS) c_loops += lane == 0 ? 1u : 0u;
    if (!slot_on[0] && !slot_on[1] && __ballot(trav) == 0ull) break;
  }

  if (!a.scanlines) {  // (with ZRT_FLAG_SCANLINES they went to the frame rows, whose sums are the totals)
    wave_add_u64(&a.counters[kDepthHits], c_depth);
    wave_add_u64(&a.counters[kReflections], c_refl);
    wave_add_u64(&a.counters[kBackground], c_bg);
  }
  if (STATS) {
    wave_add_u64(&a.counters[kRays], c_rays);
    wave_add_u64(&a.counters[kNodes], c_nodes);
    wave_add_u64(&a.counters[kTriTests], c_tri);
    wave_add_u64(&a.counters[kSphereTests], c_sph);
    wave_add_u64(&a.counters[kShades], c_shade);
    wave_add_u64(&a.counters[kTexels], c_tex);
    wave_add_u64(&a.counters[kLeaves], c_leaves);
    wave_add_u64(&a.counters[kReplays], c_replays);
    wave_add_u64(&a.counters[kTravTrips], c_trips);
    wave_add_u64(&a.counters[kLoopTrips], c_loops);
    wave_add_u64(&a.counters[kLaneSteps], c_lsteps);
    coh.flush(a.counters);
  }
}

// shade_step's first half for the list loop: a hit's scatter up
// to the direction it normalises.  Every material's new direction - and a new
// sample's camera ray - is normalised once per step for all lanes together
// (unit(), vector.zig:88-92, ~20 VALU: where the materials ran it in their own
// branches a wave paid for it up to six times per step), and a metal scatter's
// absorption test (material.zig:96-101) reads the normalised direction after it.
// Same operations on the same values as shade_step, in the same order per lane.
// pend: 0 nothing to normalise, 1 a scatter, 2 a metal scatter to be tested after.
template <bool STATS, class R>
__device__ __forceinline__ void shade_hit_a(const KArgs& a, const DevMaterial* __restrict__ mats, R& rng, int best,
                                            float best_t, const V3 o, const V3 d, bool& path_end, bool& sky, V3& L,
                                            uint32_t& c_bg, uint32_t& c_shade, uint32_t& c_tex, V3& x, V3& loc,
                                            V3& normal, uint32_t& att, uint32_t& pend) {
  pend = 0;
  if (best < 0) {
    ++c_bg;
    L = background(d);
    path_end = true;
    sky = true;
    return;
  }
  float4 sh;
  const int fb = __builtin_amdgcn_readfirstlane(best);
  if (__ballot(best != fb) == 0ull) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float4 cfloat4;
    sh = ((cfloat4*)a.shade)[fb];
#else
    sh = a.shade[fb];
#endif
  } else {
    sh = a.shade[best];
  }
  const uint32_t tag = __float_as_uint(sh.w);
  const MatReg mat = load_material(mats, tag & 0x7fffffffu);
  const uint32_t mkind = mat.kind();
  const bool need_uv = mkind != ZRT_MAT_DIELECTRIC && mat.tex_kind() == ZRT_TEX_IMAGE;
  if (STATS) {
    ++c_shade;
    c_tex += need_uv ? 1u : 0u;
  }
  loc = add(o, scale(d, best_t));
  V3 outward;
  float tu = 0.0f, tv = 0.0f;
  if (tag >> 31) {
    outward = mk(sh.x, sh.y, sh.z);
    if (need_uv) {
      const float4 p0 = a.prims[3 * best + 0];
      const float4 p1 = a.prims[3 * best + 1];
      const float4 p2 = a.prims[3 * best + 2];
      const V3 n = mk(p2.y, p2.z, p2.w);
      const float det = -dot(d, n);
      const float inv_det = inv_det_rn(det, a.tri_rcp_fast);
      const V3 ao = mk(o.x - p0.x, o.y - p0.y, o.z - p0.z);
      const V3 dao = cross(ao, d);
      tu = dot(mk(p1.z, p1.w, p2.x), dao) * inv_det;
      tv = -dot(mk(p0.w, p1.x, p1.y), dao) * inv_det;
    }
  } else {
    const float4 c = a.prims[3 * best];
    outward = scale(sub(loc, mk(c.x, c.y, c.z)), sh.x);
    if (need_uv) {
      const float theta = dev::acos_z(-outward.y);
      const float phi = dev::atan2_z(-outward.z, -outward.x) + kPi;
      tu = dev::div_known(phi, kTwoPi, kInvTwoPi);
      tv = dev::div_known(theta, kPi, kInvPi);
    }
  }
  bool front = true;
  normal = outward;
  if (dot(d, outward) > 0.0f) {
    normal = neg(outward);
    front = false;
  }
  // metal and dielectric both start from unit(d): one normalisation for the lanes of either
  V3 ud = d;
  if (mkind != ZRT_MAT_LAMBERTIAN) ud = unit(d);
  // Material.scatter (material.zig:43-129) with the operations the materials share
  // issued once for the lanes of all of them (a wave whose lanes hit two or three
  // materials otherwise runs each shared piece once per material): the correctly
  // rounded sqrt(1 - q^2) - Lambertian q = its first draw, dielectric q = cos_theta -,
  // the second uniform draw - Lambertian's r2, the dielectric's reflectance draw,
  // each lane's draws still in its own order (r1, r2, bool / one draw after its
  // Schlick term) -, reflect() for metal and reflected dielectric rays, and the
  // albedo lookup for Lambertian and metal.  The same operations on the same values
  // per lane as shade_step's per-material branches: bit-identical
  // (test_list_loops_bit_exact; C2 +2.9 %, profiles/r06/r06i).
  const bool lamb = mkind == ZRT_MAT_LAMBERTIAN, metal = mkind == ZRT_MAT_METAL;
  const bool diel = !lamb && !metal;
  float r1 = 0.0f;
  if (lamb) r1 = rand_float(rng);
  float ratio = 1.0f, cos_theta = 0.0f;
  if (diel) {
    ratio = front ? dev::rcp_rn(mat.ior()) : mat.ior();
    cos_theta = dev::fmin_z(dot(neg(ud), normal), 1.0f);
  }
  const float qv = lamb ? r1 : cos_theta;
  const float root = dev::sqrt_rn(1.0f - qv * qv);  // Lambertian rr, dielectric sin_theta
  bool refl = diel && ratio * root > 1.0f;
  float reflectance = 0.0f;
  const bool schlick = diel && !refl;
  if (schlick) {
    const float r0 = dev::div_rn(1.0f - ratio, 1.0f + ratio);
    reflectance = r0 + (1.0f - r0) * dev::pow5_z(1.0f - cos_theta);
  }
  float r2 = 0.0f;
  if (lamb || schlick) r2 = rand_float(rng);
  if (schlick) refl = reflectance > r2;
  if (lamb) {
    float sn, cs;
    dev::sincos_z(kTwoPi * r2, &sn, &cs);
    V3 hv = mk(cs * root, sn * root, r1);
    if (!rand_bool(rng)) hv.z = hv.z * -1.0f;
    x = add(normal, hv);
  } else if (metal || refl) {
    x = reflect(ud, normal);
  } else {
    x = refract(ud, normal, ratio);
  }
  att = kAttOne;
  if (!diel) att = albedo_code(mat, tag & 0x7fffffffu, tu, tv);  // (metal: used only when not absorbed)
  pend = metal ? 2u : 1u;
}

// ---------------------------------------------------------------------------
// The surface-list loop with per-lane work items (MODE 6; raytrace.zig:71-81
// without a BVH, config C2).  Every ray of a list scene costs the same - all
// n_list surfaces, read through the scalar cache - so the coherence that makes
// the lockstep loop win on a BVH buys nothing here, while its waits cost most
// of the lanes: a wave that steps sample by sample waits for its longest path
// (C2: 2.14 rays per sample, glass paths up to depth 30; VALU lane utilisation
// 0.31).  Here a work item is one (pixel, chunk) - the 64 items of a unit are
// the 64 pixels of its tile - and each lane runs its own item's samples in
// order and takes the next item as soon as it is done: the wave claims a unit
// (one atomic) and hands its pixels to its lanes as they free up (ballot +
// mbcnt rank), so no lane waits for another.  The chunk's sum is the same
// sequential sum in the same slot, so images are bit-identical to the other
// loops'.
// ---------------------------------------------------------------------------
template <int PRNG, bool STATS>
__device__ __forceinline__ void render_loop_list(const KArgs& a) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  lds_u32* att_l = (lds_u32*)(lds_raw + a.lds_att_off) + threadIdx.x;  // [row][lane] att codes
  // (the host planned the material table into LDS, as for the lockstep loop: LDS-typed reads)
  float4* mats_l = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
  fill_lds_mats(a, mats_l);
  const DevMaterial* mats = reinterpret_cast<const DevMaterial*>(mats_l);
#if defined(__HIP_DEVICE_COMPILE__)
  typedef const __attribute__((address_space(4))) float4 cfloat4;  // the list is wave-uniform: scalar loads
  cfloat4* cprims = (cfloat4*)a.prims;
  cfloat4* cshade = (cfloat4*)a.shade;
#else
  const float4* cprims = a.prims;
  const float4* cshade = a.shade;
#endif
  const int lane = (int)__lane_id();
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;

  bool has = false, in_sample = false;  // this lane holds an item / one of its samples is under way
  bool exhausted = false;               // wave-uniform: the unit counter ran out
  // the wave's current unit (wave-uniform): tile, chunk, corner, next pixel to hand out (64: none left)
  uint32_t u_lt = 0, u_chunk = 0, u_x0 = 0, u_y0 = 0, u_next = 64;
  uint32_t sample = 0, s_end = 0, slot = 0, px = 0, py = 0;
  float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
  V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
  uint32_t depth_left = 0;
  Rng<PRNG> rng;
  rng.init(0);
  uint32_t c_rays = 0, c_refl = 0, c_bg = 0, c_depth = 0, c_tri = 0, c_sph = 0, c_shade = 0, c_tex = 0;
  uint32_t c_loops = 0, c_lsteps = 0;
  Coh coh;  // STATS
  for (;;) {
    // ---- refill: the lanes without an item take the next pixels of the wave's
    // current unit (ballot + mbcnt rank); a unit runs dry -> the next one, one
    // atomic per 64 items (an atomic per refill step ran the C2 frame at a
    // quarter of the rate: one global counter for every wave's every step)
    const uint64_t need = __ballot(!has);
    if (need != 0ull && !(exhausted && u_next >= 64u)) {
      const uint32_t rank =
          (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(need >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need, 0u));
      const uint32_t cnt = (uint32_t)__builtin_popcountll(need);
      uint32_t taken = 0;  // lanes served so far (by rank)
#pragma unroll 1
      for (int pass = 0; pass < 2 && taken < cnt; ++pass) {
        if (u_next >= 64u) {  // the wave's unit is handed out: claim the next one
          if (exhausted) break;
          uint32_t u = 0;
          if (lane == 0) u = atomicAdd(a.work_counter, 1u);
          u = __builtin_amdgcn_readfirstlane(u);
          if (u >= a.total_work) {
            exhausted = true;
            break;
          }
          const uint32_t ord = u / a.n_chunks;
          u_chunk = u - ord * a.n_chunks;
          u_lt = a.tile_order ? a.tile_order[ord] : ord;
          const uint32_t t = u_lt * a.world + a.rank;  // local tile lt = global tile lt*world + rank
          u_x0 = (t % a.tiles_x) * 8u;
          u_y0 = (t / a.tiles_x) * 8u;
          u_next = 0;
        }
        const uint32_t take = min(cnt - taken, 64u - u_next);
        if (!has && rank >= taken && rank < taken + take) {
          const uint32_t p = u_next + (rank - taken);
          px = u_x0 + (p & 7u);
          py = u_y0 + (p >> 3);
          if (px < a.xbound && py < a.height) {  // off-frame pixels: nothing (finalize writes black)
            has = true;
            in_sample = false;
            sample = u_chunk * a.chunk;
            s_end = min(sample + a.chunk, a.spp);
            slot = u_chunk * a.n_slots + u_lt * 64u + p;
            acc_r = acc_g = acc_b = 0.0f;
          }
        }
        taken += take;
        u_next += take;
      }
    }
    if (__ballot(has) == 0ull) {
      if (exhausted && u_next >= 64u) break;
      continue;  // (every lane drew an off-frame pixel)
    }
    if (STATS) {
      c_loops += lane == 0 ? 1u : 0u;
      c_lsteps += has ? 1u : 0u;
    }
    if (!has) continue;
    // ---- a new sample: jitter + Camera.getRay (raytrace.zig:173-175)
    if (!in_sample) {
      const uint64_t offset = (uint64_t)py * a.width + px;
      rng.init(((offset << 16) | (uint64_t)sample) + a.seed_mix);
      const float u = dev::div_known((float)px + rand_float(rng) - 0.5f, a.f_width, a.inv_width);
      const float v = dev::div_known((float)py + rand_float(rng) - 0.5f, a.f_height, a.inv_height);
      o = mk(a.org[0], a.org[1], a.org[2]);
      d = unit(sub(add(add(mk(a.llc[0], a.llc[1], a.llc[2]), scale(mk(a.hor[0], a.hor[1], a.hor[2]), u)),
                       scale(mk(a.ver[0], a.ver[1], a.ver[2]), v)),
                   o));
      depth_left = a.max_depth;
      in_sample = true;
    }
    // ---- one rayColor step (raytrace.zig:62-100)
    bool path_end = false, sky = false;
    V3 L = mk(0.0f, 0.0f, 0.0f);
    const uint32_t dh0 = c_depth, rf0 = c_refl, bg0 = c_bg;
    const AttRows ar{att_l, kBlock, gl, a.n_lanes};
    V3 x = mk(0.0f, 0.0f, 0.0f), loc = x, nrm = x;  // the direction to normalise, hit, normal
    uint32_t att = 0, pend = 0;
    if (depth_left == 0) {
      ++c_depth;
      path_end = true;
    } else {
      if (STATS) ++c_rays;
      RayT r;
      r.ox = o.x; r.oy = o.y; r.oz = o.z;
      r.dx = d.x; r.dy = d.y; r.dz = d.z;
      r.rcp_det = a.tri_rcp_fast;
      r.gm = a.graze_m;
      r.gl = a.graze_leaf;
      r.gk = a.guard;
      inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
      float best_t = __builtin_inff();
      int best = -1;
      for (uint32_t i = 0; i < a.n_list; ++i) {  // surfaces in list order, t_max shrinking
        const uint32_t tag = __float_as_uint(cshade[i].w);
        if (tag >> 31) {
          if (STATS) ++c_tri;
          tri_test_v<false>(cprims[3 * i], cprims[3 * i + 1], cprims[3 * i + 2], (int)i, r, best_t, best);
        } else {
          if (STATS) ++c_sph;
          sphere_test<false>(cprims[3 * i], (int)i, r, best_t, best);
        }
      }
      // one unit() per step for every new direction (scatters and camera rays): shade_hit_a
      shade_hit_a<STATS>(a, mats, rng, best, best_t, o, d, path_end, sky, L, c_bg, c_shade, c_tex, x, loc, nrm, att,
                         pend);
    }
    bool cam = false;  // the item's next sample starts in this step
    if (path_end) {
      const V3 col = sky ? att_product<STATS>(a, mats, ar, a.max_depth - depth_left, L, coh) : L;
      acc_r += col.x;
      acc_g += col.y;
      acc_b += col.z;
      in_sample = false;
      if (++sample == s_end) {  // the chunk's sequential sum, in its [chunk][pixel slot] place
        a.partial[slot] = make_float4(acc_r, acc_g, acc_b, 0.0f);
        has = false;
      } else {  // the next sample's jitter + Camera.getRay (raytrace.zig:173-175)
        const uint64_t offset = (uint64_t)py * a.width + px;
        rng.init(((offset << 16) | (uint64_t)sample) + a.seed_mix);
        const float u = dev::div_known((float)px + rand_float(rng) - 0.5f, a.f_width, a.inv_width);
        const float v = dev::div_known((float)py + rand_float(rng) - 0.5f, a.f_height, a.inv_height);
        x = sub(add(add(mk(a.llc[0], a.llc[1], a.llc[2]), scale(mk(a.hor[0], a.hor[1], a.hor[2]), u)),
                    scale(mk(a.ver[0], a.ver[1], a.ver[2]), v)),
                mk(a.org[0], a.org[1], a.org[2]));
        cam = true;
        in_sample = true;
      }
    }
    if (pend != 0u || cam) {  // every new direction of the step, normalised together
      const V3 nd = unit(x);
      if (cam) {
        o = mk(a.org[0], a.org[1], a.org[2]);
        d = nd;
        depth_left = a.max_depth;
      } else if (pend == 1u || dot(nd, nrm) > 0.0f) {  // scattered (material.zig:71-128)
        ++c_refl;
        if (depth_left > 1) {  // (shade_step: an attenuation pushed at depth 1 is never read)
          const uint32_t i = a.max_depth - depth_left;
          if (i < a.att_lds_rows) {
            ar.lds[i * ar.lds_stride] = att;
          } else {
            const uint64_t k = (uint64_t)(i - a.att_lds_rows) * ar.g_stride + ar.g_index;
            if (row_ok<STATS>(a, k, a.att_cap)) a.att[k] = att;
            if (STATS) ++coh.attw;
          }
        }
        o = loc;
        d = nd;
        --depth_left;
      } else {  // a metal scatter absorbed: the path ends black (its next sample starts next step)
        acc_r += 0.0f;
        acc_g += 0.0f;
        acc_b += 0.0f;
        in_sample = false;
        if (++sample == s_end) {
          a.partial[slot] = make_float4(acc_r, acc_g, acc_b, 0.0f);
          has = false;
        }
      }
    }
    if (a.scanlines) {  // this lane's item is one pixel: its events go to its row (raytrace.zig:184)
      scanline_add(a, py, 0, c_depth - dh0);
      scanline_add(a, py, 1, c_refl - rf0);
      scanline_add(a, py, 2, c_bg - bg0);
    }
  }
  if (!a.scanlines) {  // (with ZRT_FLAG_SCANLINES they went to the frame rows, whose sums are the totals)
    wave_add_u64(&a.counters[kDepthHits], c_depth);
    wave_add_u64(&a.counters[kReflections], c_refl);
    wave_add_u64(&a.counters[kBackground], c_bg);
  }
  if (STATS) {
    wave_add_u64(&a.counters[kRays], c_rays);
    wave_add_u64(&a.counters[kTriTests], c_tri);
    wave_add_u64(&a.counters[kSphereTests], c_sph);
    wave_add_u64(&a.counters[kShades], c_shade);
    wave_add_u64(&a.counters[kTexels], c_tex);
    wave_add_u64(&a.counters[kLoopTrips], c_loops);
    wave_add_u64(&a.counters[kLaneSteps], c_lsteps);
    coh.flush(a.counters);
  }
}

#ifndef ZRT_ATT_ROWS_LIST
#define ZRT_ATT_ROWS_LIST 24  // list loops (MODE 0 / 6): attenuation rows kept in LDS (as many as their 6-block share holds)
#endif
#ifndef ZRT_ATT_ROWS_LOCK
#define ZRT_ATT_ROWS_LOCK 4  // lockstep FAST loop: attenuation rows kept in LDS (4 KiB per block, beside its lane state)
#endif
#ifndef ZRT_ATT_ROWS_WF
#define ZRT_ATT_ROWS_WF 12  // wavefront loop: attenuation rows kept in LDS (12 KiB per block, as 4 rows of 3 floats were)
#endif
#ifndef ZRT_WAVES_WF
#define ZRT_WAVES_WF 4  // wavefront loop (MODE 4)
#endif

#ifndef ZRT_WAVES_POOL
#define ZRT_WAVES_POOL 4  // path-pool loop (MODE 5)
#endif
#ifndef ZRT_ATT_ROWS_POOL
#define ZRT_ATT_ROWS_POOL 3  // path-pool loop: attenuation rows kept in LDS per path (2 KiB per row per block)
#endif

template <int MODE, int PRNG, bool STATS, class StackT, bool LEAN = false, bool ONE_SPHERE = false>
__global__ void __launch_bounds__(kBlock, MODE == 5 || MODE == 7 || MODE == 8 || MODE == 9 ? ZRT_WAVES_POOL
                                          : MODE == 4 ? ZRT_WAVES_WF
                                          : MODE == 3 ? ZRT_WAVES_WIDE
                                          : MODE == 0 || MODE == 6 ? ZRT_WAVES_LIST
                                                      : ZRT_WAVES_PER_SIMD)
    render_kernel(const KArgs a) {
  static_assert(!ONE_SPHERE || MODE == 3, "the one-sphere kernels are the lockstep FAST loop's");
  if constexpr (MODE == 6) render_loop_list<PRNG, STATS>(a);
  else if constexpr (MODE == 5) render_loop_pool<PRNG, STATS, StackT, false>(a);
  else if constexpr (MODE == 7) render_loop_pool<PRNG, STATS, StackT, true>(a);  // with the grazing-triangle guard
  else if constexpr (MODE == 8) render_loop_pool<PRNG, STATS, StackT, false, true>(a);  // compressed nodes
  else if constexpr (MODE == 9) render_loop_pool<PRNG, STATS, StackT, true, true>(a);   // compressed, guarded
  else if constexpr (MODE == 4) render_loop_wf<PRNG, STATS, StackT>(a);
  else render_loop<MODE, PRNG, STATS, StackT, false, LEAN, ONE_SPHERE>(a);
}

// The scheduling probe (FAST traversal): the same loop over a few samples per
// pixel, one unit per tile, recording each tile's cost (a.unit_cost); its own
// symbol so profiles keep it apart from the render launches.
template <int PRNG, class StackT>
__global__ void __launch_bounds__(kBlock, ZRT_WAVES_WIDE) schedule_probe_kernel(const KArgs a) {
  render_loop<3, PRNG, false, StackT, true>(a);
}

// The sky kernel: the tiles the host proved all sky (tile_class.cpp: no primary ray
// of the tile can hit anything), with no traversal.  Every sample of such a tile is
// one camera ray that ends in the background, so what is left of render_loop's
// sample is its seed, its two draws, Camera.getRay's unit(), background(d) and the
// add - the same expressions in the same order, so the chunk sums are the render
// loop's bit for bit (att_product over zero rows returns L itself).  One wave per
// unit (tile x chunk) of a.tile_order (the sky list), lane p = pixel p, units dealt
// round-robin; the sums go to the same partial[chunk][slot], the samples to
// kBackground (STATS: and to kRays).  No LDS, no scene arrays.
template <int PRNG, bool STATS>
__global__ void __launch_bounds__(kBlock) sky_kernel(const KArgs a) {
  const uint32_t lane = __lane_id();
  const uint32_t n_waves = gridDim.x * (kBlock / 64);
  const V3 llc = mk(a.llc[0], a.llc[1], a.llc[2]);
  const V3 hor = mk(a.hor[0], a.hor[1], a.hor[2]);
  const V3 ver = mk(a.ver[0], a.ver[1], a.ver[2]);
  const V3 o = mk(a.org[0], a.org[1], a.org[2]);
  uint32_t c_bg = 0;
  for (uint32_t u = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); u < a.total_work; u += n_waves) {
    const uint32_t ord = u / a.n_chunks, g = u - ord * a.n_chunks;
    const uint32_t lt = a.tile_order[ord];
    const uint32_t t = lt * a.world + a.rank;
    const uint32_t px = (t % a.tiles_x) * 8u + (lane & 7u), py = (t / a.tiles_x) * 8u + (lane >> 3);
    const uint32_t first = g * a.chunk, end = min(first + a.chunk, a.spp);
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    if (px < a.xbound && py < a.height) {  // off-frame lanes stay idle (finalize writes black)
      const uint64_t offset = (uint64_t)py * a.width + px;
      for (uint32_t sample = first; sample < end; ++sample) {
        Rng<PRNG> rng;
        rng.init(((offset << 16) | (uint64_t)sample) + a.seed_mix);
        const float su = dev::div_known((float)px + rand_float(rng) - 0.5f, a.f_width, a.inv_width);
        const float sv = dev::div_known((float)py + rand_float(rng) - 0.5f, a.f_height, a.inv_height);
        const V3 d = unit(sub(add(add(llc, scale(hor, su)), scale(ver, sv)), o));
        const V3 L = background(d);
        acc_r += L.x;
        acc_g += L.y;
        acc_b += L.z;
      }
      c_bg += end - first;
    }
    a.partial[g * a.n_slots + lt * 64u + lane] = make_float4(acc_r, acc_g, acc_b, 0.0f);
  }
  wave_add_u64(&a.counters[kBackground], c_bg);
  if (STATS) wave_add_u64(&a.counters[kRays], c_bg);
}

// The closest hit of one ray whose direction Ray.init has normalised: the
// top-level query of rayColor (raytrace.zig:71-81, t_min 0.001, t_max shrinking)
// through the same traversal code as the render loop.  best < 0: a miss.
template <int MODE, class StackT>
__device__ __forceinline__ void closest_hit(const KArgs& a, const V3 o, const V3 d, StackT* stk, float4* lds_top,
                                            uint32_t gl, float& best_t, int& best) {
  RayT r;
  r.ox = o.x; r.oy = o.y; r.oz = o.z;
  r.dx = d.x; r.dy = d.y; r.dz = d.z;
  r.rcp_det = a.tri_rcp_fast;
  r.gm = a.graze_m;
  r.gl = a.graze_leaf;
  r.gk = a.guard;
  inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
  best_t = __builtin_inff();
  best = -1;
  uint32_t c_nodes = 0, c_leaves = 0, c_tri = 0, c_sph = 0;
  if (MODE == 0) {
    for (uint32_t i = 0; i < a.n_list; ++i) {  // surfaces in list order
      if (__float_as_uint(a.shade[i].w) >> 31) tri_test<false>(a.prims, (int)i, r, best_t, best);
      else sphere_test<false>(a.prims[3 * i], (int)i, r, best_t, best);
    }
  } else if (MODE == 3) {
    uint32_t c_replays = 0;
    Coh coh;
    traverse_wide<false, StackT, true>(a, r, stk, lds_top, gl, best_t, best, c_nodes, c_leaves, c_tri, c_sph, c_replays,
                                       coh);
  } else if (MODE == 8) {  // compressed nodes
    uint32_t c_replays = 0;
    Coh coh;
    traverse_wide_q<false, StackT>(a, r, stk, lds_top, gl, best_t, best, c_nodes, c_leaves, c_tri, c_sph, c_replays,
                                   coh);
  } else {
    traverse_bvh<MODE == 1, false>(a, r, stk, best_t, best, c_nodes, c_tri, c_sph);
  }
}

// Closest hit of a batch of rays (zrt_trace), one lane per ray.  Ray.init
// normalises the direction (ray.zig:11-13).  Result: t (+inf on a miss) and the
// device slot.
template <int MODE, class StackT>
__global__ void __launch_bounds__(kBlock) trace_kernel(const KArgs a, const float* __restrict__ rays, uint32_t n,
                                                       float* __restrict__ out_t, int32_t* __restrict__ out_slot) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if ((MODE == 3 || MODE == 8) && !layout_ok(a)) return;
  if ((MODE == 3 || MODE == 8)) fill_lds_top(a, lds_top);
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  if (gl >= n) return;
  const float* q = rays + 6ull * gl;
  const V3 d = unit(mk(q[3], q[4], q[5]));
  float best_t;
  int best;
  closest_hit<MODE, StackT>(a, mk(q[0], q[1], q[2]), d, stk, lds_top, gl, best_t, best);
  out_t[gl] = best < 0 ? __builtin_inff() : best_t;
  out_slot[gl] = best;
}

// The end of a resident closest-hit query (zrt_ctx_trace) behind trace_kernel: the
// device slot mapped to the index in the reference's list (slot_prim), or, after a
// launch that set its error flag (a traversal stack overflow), t = NaN and prim = -1.
__global__ void trace_finish_kernel(float* __restrict__ t, int32_t* __restrict__ prim, uint32_t n,
                                    const uint32_t* __restrict__ slot_prim,
                                    const unsigned long long* __restrict__ error_flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (*error_flag != 0ull) {
    t[i] = __builtin_nanf("");
    prim[i] = -1;
    return;
  }
  const int32_t s = prim[i];
  prim[i] = s < 0 ? -1 : (int32_t)slot_prim[s];
}

// ---------------------------------------------------------------------------
// Any-hit (zrt_ctx_occluded; DESIGN.md §5 "Ray queries"): is some primitive hit
// in (0.001, t_max) as rayColor's surface loop (raytrace.zig:71-81) started with
// t_max would find it.  Under the BVH (bvh.zig:187-205 with a t_max that never
// shrinks before the answer is "yes") that is: a primitive whose own leaf, and
// every ancestor of it, passes hitAabb(ray, 0.001, t_max) and whose hit test
// passes with the strict bounds t_min < t < t_max.
// ---------------------------------------------------------------------------
// One primitive against the fixed interval: the reference's own tests
// (sphere.zig:43/57, triangle.zig:62), nothing shrinking.
__device__ __forceinline__ bool prim_in_range(const float4* __restrict__ prims, int ref, const RayT& r, float t_max) {
  float t = t_max;
  int b = -1;
  uint32_t c_tri = 0, c_sph = 0;
  prim_test<false, false>(prims, ref, r, t, b, c_tri, c_sph);
  return b >= 0;
}

// The literal traversal: reference_replay started at t_max, leaving at the first
// hit.  Every box goes through the reference's loose test against the fixed t_max,
// left first.  narrow: boxes the ray does not cross are culled too (the narrowed
// test with the grazing slack and the guard; never a box holding a sphere) - they
// hold no hit, so the answer is the same; false: the reference's
// test alone.  Stack rows as the replay's: a.lds_rows in LDS, the rest in stack_ovf.
template <class StackT>
__device__ __forceinline__ bool anyhit_literal(const KArgs& a, const RayT& r, StackT* __restrict__ stk, uint32_t gl,
                                            float t_max, bool narrow) {
  const uint32_t rows = a.lds_rows, cap = a.ref_stack;
  StackT* __restrict__ ovf = reinterpret_cast<StackT*>(a.stack_ovf) + gl;
  const float slack = ray_slack(r, a.scene_extent, ray_m(r));
  const float gw = r.gk > 0.0f ?guard_grow(a, r) : 0.0f;
  stk[0] = 0;
  uint32_t sp = 1;
  while (sp > 0) {
    --sp;
    const int idx = sp < rows ? (int)stk[sp * kBlock] : (int)ovf[(size_t)(sp - rows) * a.n_lanes];
    const float4 lo = a.nodes[2 * idx], hi = a.nodes[2 * idx + 1];
    float e;
    if (!box_test<true>(lo, hi, r, t_max, &e, slack, narrow && a.ref_sph[idx] == 0, gw)) continue;
    const int left = as_int(lo.w), right = as_int(hi.w);
    if (left < 0) {
      if (prim_in_range(a.prims, left, r, t_max)) return true;
      if (right != left && prim_in_range(a.prims, right, r, t_max)) return true;
    } else if (sp + 2 <= cap) {
      const StackT v[2] = {(StackT)right, (StackT)left};
#pragma unroll
      for (uint32_t j = 0; j < 2; ++j) {
        if (sp + j < rows) stk[(sp + j) * kBlock] = v[j];
        else ovf[(size_t)(sp + j - rows) * a.n_lanes] = v[j];
      }
      sp += 2;
    } else {
      atomicOr(a.error_flag, kErrOverflow);
    }
  }
  return false;
}

// The acceptance rule: a primitive hit in (0.001, t_max) found by a traversal that
// culls against t_max * kOpen counts only if its own reference leaf passes the
// reference's loose test at exactly t_max.  The leaf's ancestors need no test: the
// loose test is monotone under box containment, also with the min(t1, t_max) clamp.
// A flat leaf fails it, as the reference never opens one.
__device__ __forceinline__ bool leaf_accepts(const float4 lo, const float4 hi, const RayT& r, float t_max) {
  float e;
  return box_test<false>(lo, hi, r, t_max, &e);
}

// BINARY: near-first over the reference nodes, every box through binary_test against
// the fixed t_max * kOpen + slack with the guard on; a leaf's candidates count when
// the leaf accepts.  A popped node's box passed that same test when it was pushed.
template <class StackT>
__device__ __forceinline__ bool anyhit_binary(const KArgs& a, const RayT& r, StackT* __restrict__ stk, uint32_t gl,
                                              float t_max) {
  if (!ray_origin_ok(a, r)) return anyhit_literal<StackT>(a, r, stk, gl, t_max, false);
  const float slack = ray_slack(r, a.scene_extent, ray_m(r));
  const float gw = r.gk > 0.0f ?guard_grow(a, r) : 0.0f;
  const float tb = t_max * kOpen + slack;
  const uint32_t cap = a.stack_depth;
  uint32_t sp = 0;
  float e;
  float4 lo = a.nodes[0], hi = a.nodes[1];
  if (!binary_test(a, 0, lo, hi, r, tb, &e, slack, gw)) return false;
  for (;;) {
    const int left = as_int(lo.w), right = as_int(hi.w);
    if (left < 0) {
      if ((prim_in_range(a.prims, left, r, t_max) || (right != left && prim_in_range(a.prims, right, r, t_max))) &&
          leaf_accepts(lo, hi, r, t_max))
        return true;
    } else {
      const float4 l0 = a.nodes[2 * left], l1 = a.nodes[2 * left + 1];
      const float4 r0 = a.nodes[2 * right], r1 = a.nodes[2 * right + 1];
      float el, er;
      const bool hl = binary_test(a, left, l0, l1, r, tb, &el, slack, gw);
      const bool hr = binary_test(a, right, r0, r1, r, tb, &er, slack, gw);
      if (hl && hr) {
        const bool rfirst = er < el;
        if (sp < cap) stk[(sp++) * kBlock] = (StackT)(rfirst ? left : right);
        else atomicOr(a.error_flag, kErrOverflow);  // too deep for the stack: the subtree is dropped (flagged)
        lo = rfirst ? r0 : l0;
        hi = rfirst ? r1 : l1;
        continue;
      }
      if (hl) { lo = l0; hi = l1; continue; }
      if (hr) { lo = r0; hi = r1; continue; }
    }
    if (sp == 0) return false;
    const int idx = stk[(--sp) * kBlock];
    lo = a.nodes[2 * idx];
    hi = a.nodes[2 * idx + 1];
  }
}

// FAST, over the full 128-B wide nodes: wide_iter with the "best" held at the fixed
// t_max - no near-tie tracking read, no order hazard, no replay of the closest hit.
// After every node the lane looks at what the node's leaves left in (best_t, best):
// a candidate whose reference leaf accepts is the answer.  A rejected candidate may
// have hidden a later primitive of the same node behind its smaller t, so that ray
// goes through the literal traversal (narrowed: it holds the same hits) - rare: the
// near-miss spheres and the hazard scene's sphere are where it happens.  Rays whose
// origin lies outside the bound, degenerate rays, and a t_max wide_iter's state
// cannot carry (negative or NaN: the sign of best_t is its near-tie flag) take the
// literal traversal alone.
template <class StackT>
__device__ __forceinline__ bool anyhit_wide(const KArgs& a, const RayT& r, StackT* __restrict__ stk,
                                            const float4* __restrict__ lds_top, uint32_t gl, float t_max) {
  const bool far = !ray_origin_ok(a, r) || ray_degenerate(r);
  bool literal = far || !(t_max >= 0.0f);
  if (!literal) {
    const WideView v = wide_view(a, r, lds_top);
    uint32_t sp = 0;
    const float4* q = v.top;
    WideNode w;
    const OctSigns os(r);
    wide_load(q, os.sx, os.sy, os.sz, w);
    uint32_t c_nodes = 0, c_leaves = 0, c_tri = 0, c_sph = 0;
    Coh coh;
    bool more = true;
    while (more) {
      float best_t = t_max;
      int best = -1;
      more = wide_iter<false, StackT, true, true, true>(a, r, v, stk, gl, w, q, sp, best_t, best, c_nodes, c_leaves,
                                                        c_tri, c_sph, coh);
      if (best >= 0) {
        const uint32_t leaf = a.leaf_of_slot[best];
        if (leaf_accepts(a.nodes[2 * leaf], a.nodes[2 * leaf + 1], r, t_max)) return true;
        literal = true;
        break;
      }
    }
  }
  return literal ? anyhit_literal<StackT>(a, r, stk, gl, t_max, !far) : false;
}

// The any-hit of one ray whose direction Ray.init has normalised, through the
// launch's traversal (anyhit_kernel and ao_kernel): gl is the lane's index in the
// launch, which owns stack column gl of the overflow rows.
template <int MODE, class StackT>
__device__ __forceinline__ bool anyhit_ray(const KArgs& a, const V3 o, const V3 d, float t_max, StackT* __restrict__ stk,
                                           const float4* __restrict__ lds_top, uint32_t gl) {
  RayT r;
  r.ox = o.x; r.oy = o.y; r.oz = o.z;
  r.dx = d.x; r.dy = d.y; r.dz = d.z;
  r.rcp_det = a.tri_rcp_fast;
  r.gm = a.graze_m;
  r.gl = a.graze_leaf;
  r.gk = a.guard;
  inv_dir(d.x, d.y, d.z, r.ix, r.iy, r.iz);
  bool hit = false;
  if (MODE == 0) {
    for (uint32_t i = 0; i < a.n_list && !hit; ++i) {  // surfaces in list order, leaving at the first hit
      float t = t_max;
      int b = -1;
      if (__float_as_uint(a.shade[i].w) >> 31) tri_test<false>(a.prims, (int)i, r, t, b);
      else sphere_test<false>(a.prims[3 * i], (int)i, r, t, b);
      hit = b >= 0;
    }
  } else if (MODE == 3) {
    hit = anyhit_wide<StackT>(a, r, stk, lds_top, gl, t_max);
  } else if (MODE == 1) {
    hit = anyhit_binary<StackT>(a, r, stk, gl, t_max);
  } else {
    hit = anyhit_literal<StackT>(a, r, stk, gl, t_max, false);
  }
  return hit;
}

// One ray per lane; a lane that has its answer stops traversing, the wave ends when
// all have.  t_max: per ray, or null = +inf.  out: 1 occluded / 0 not.
template <int MODE, class StackT>
__global__ void __launch_bounds__(kBlock) anyhit_kernel(const KArgs a, const float* __restrict__ rays,
                                                        const float* __restrict__ t_max_in, uint32_t n,
                                                        uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  if (gl >= n) return;
  const float* q = rays + 6ull * gl;
  const V3 d = unit(mk(q[3], q[4], q[5]));
  const float t_max = t_max_in ? t_max_in[gl] : __builtin_inff();
  const bool hit = anyhit_ray<MODE, StackT>(a, mk(q[0], q[1], q[2]), d, t_max, stk, lds_top, gl);
  out[gl] = hit ? (uint8_t)1 : (uint8_t)0;
}

// An any-hit launch that set its error flag leaves 0xFF in every byte.
__global__ void anyhit_error_kernel(uint8_t* __restrict__ out, uint32_t n,
                                    const unsigned long long* __restrict__ error_flag) {
  if (*error_flag == 0ull) return;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (uint8_t)0xFF;
}

// ---------------------------------------------------------------------------
// Ambient occlusion (zrt_ctx_ao; zrt.h "ambient occlusion"): the rays
// Lambertian.scatter shoots from the first hits of a feature buffer, through the
// any-hit above, counted per pixel.  No ray is stored.
// ---------------------------------------------------------------------------
// A pixel as the AO kernels see it.
enum : uint32_t { kAoOff = 0, kAoOutside = 1, kAoMiss = 2, kAoPoison = 3, kAoHit = 4 };
__device__ __forceinline__ uint32_t ao_classify(const float4* __restrict__ feat, uint64_t pix) {
  if (__float_as_uint(reinterpret_cast<const float*>(feat)[8ull * pix + 7]) == 0u) return kAoMiss;
  const float4 f = feat[2ull * pix];
  return (f.x != f.x || f.y != f.y || f.z != f.z || f.w != f.w) ? kAoPoison : kAoHit;
}
// A pixel's result (zrt.h): c the samples of this call that got away.
__device__ __forceinline__ void ao_store(const AoArgs& g, uint32_t kind, uint32_t c, uint64_t pix,
                                         uint32_t* __restrict__ clear, float* __restrict__ ao) {
  uint32_t v = 0u;
  float f = 0.0f;
  if (kind != kAoOutside) {
    const uint32_t old = g.accumulate ? clear[pix] : 0u;
    if (kind == kAoPoison || old == 0xFFFFFFFFu) {
      v = 0xFFFFFFFFu;
      f = __builtin_nanf("");
    } else {
      v = old + (kind == kAoMiss ? g.n_samples : c);
      f = (float)v / (float)(g.accumulate ? g.first_sample + g.n_samples : g.n_samples);  // IEEE `/`
    }
  }
  clear[pix] = v;
  if (ao) ao[pix] = f;
}

// A lane is one (pixel, sample): ray i = slot * n_samples + s, slot the pixel's place in
// the 8x8 tile order of features_kernel, so a pixel's samples sit on adjacent lanes and
// a wave's rays share origins.  The grid is bounded (zrt::plan_ao): a block loops over
// its groups of kBlock rays, and its lanes keep one stack column each (gl) however many
// rays the frame has.  Rays and pixels are indexed in 64 bits.  A wave's first ray is
// wave-uniform, so the one 64-bit division is scalar; lanes divide 32-bit offsets.
// Lanes of misses, poisoned pixels and pixels outside D traverse nothing.
// The reduction: one ballot of "got away" per wave; the first lane of each run of lanes
// on one pixel takes the popcount of its run.  in_wave (n_samples divides 64): the run is
// the whole pixel and that lane writes the result; else it adds the run's count onto the
// zeroed plane (one vector atomic per pixel and wave) and ao_finish_kernel writes.
// FAST is built for 4 waves per SIMD (128 VGPRs), anyhit_kernel's occupancy: left to itself the
// compiler takes 131 and drops to 3.
template <int MODE, int PRNG, class StackT>
__global__ void __launch_bounds__(kBlock, MODE == 3 ? 4 : 1) ao_kernel(const KArgs a, const AoArgs g, const float4* __restrict__ feat,
                                                    uint32_t* __restrict__ clear, float* __restrict__ ao,
                                                    uint32_t* __restrict__ plane) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t n = g.n_samples;
  const V3 llc = mk(a.llc[0], a.llc[1], a.llc[2]);
  const V3 hor = mk(a.hor[0], a.hor[1], a.hor[2]);
  const V3 ver = mk(a.ver[0], a.ver[1], a.ver[2]);
  const V3 o = mk(a.org[0], a.org[1], a.org[2]);
  uint32_t round = 0;
  for (uint64_t base = 0; base < g.n_groups; base += gridDim.x, ++round) {
    // round k hands group base + j to block (j - k * rotate) mod grid: a block's groups wander over the
    // frame's columns instead of lining up in one stripe of tiles (grid groups are often whole tile rows)
    const uint64_t grp = base + (blockIdx.x + (uint64_t)round * g.rotate) % gridDim.x;
    if (grp >= g.n_groups) continue;
    const uint64_t i0 = grp * kBlock + wave * 64u;  // the wave's first ray
    const uint64_t slot0 = i0 / n;
    const uint32_t k = (uint32_t)(i0 - slot0 * n) + lane;  // < n + 64
    const uint32_t dq = k / n;
    const uint32_t s = k - dq * n;
    const uint64_t slot = slot0 + dq;
    const uint32_t tile = (uint32_t)(slot >> 6), p = (uint32_t)slot & 63u;
    const uint32_t px = (tile % g.tiles_w) * 8u + (p & 7u), py = (tile / g.tiles_w) * 8u + (p >> 3);
    const uint64_t pix = (uint64_t)py * a.width + px;
    uint32_t kind = kAoOff;
    if (slot < g.n_slots && px < a.width && py < a.height) kind = px < a.xbound ? ao_classify(feat, pix) : kAoOutside;
    bool away = false;
    if (kind == kAoHit) {
      const float4 f = feat[2ull * pix];
      const float u = (float)px / a.f_width;  // IEEE `/`, as features_kernel
      const float v = (float)py / a.f_height;
      const V3 dir = unit(sub(add(add(llc, scale(hor, u)), scale(ver, v)), o));
      const V3 loc = add(o, scale(dir, f.w));  // ray.zig:14-16
      V3 hv;
      {  // randomUnitVector (sample.zig:47-61) on the sample's own stream: dead before the traversal
        Rng<PRNG> rng;
        rng.init(((pix << 16) | (uint64_t)(g.first_sample + s)) + a.seed_mix);
        const float r1 = rand_float(rng);
        const float r2 = rand_float(rng);
        const float rr = dev::sqrt_rn(1.0f - r1 * r1);
        float sn, cs;
        dev::sincos_z(kTwoPi * r2, &sn, &cs);
        hv = mk(cs * rr, sn * rr, r1);
        if (!rand_bool(rng)) hv.z = hv.z * -1.0f;
      }
      const V3 d = unit(add(mk(f.x, f.y, f.z), hv));  // material.zig:73, Ray.init
      away = !anyhit_ray<MODE, StackT>(a, loc, d, g.radius, stk, lds_top, gl);
    }
    const uint64_t bal = __ballot(away);
    const uint32_t lo = s > lane ? 0u : lane - s;              // the run of this pixel's lanes in the wave
    const uint32_t hi = min(63u, lane + (n - 1u - s));
    const uint64_t run = (~0ull >> (63u - (hi - lo))) << lo;
    const uint32_t c = (uint32_t)__popcll(bal & run);
    if (lane == lo && kind != kAoOff) {
      if (g.in_wave) ao_store(g, kind, c, pix, clear, ao);
      else if (c) atomicAdd(&plane[pix], c);
    }
  }
}

// Behind ao_kernel, one lane per pixel of the frame.  After a launch that set its error
// flag (a traversal stack overflow): 0xFFFFFFFF / NaN in every pixel of D.  Else, after
// the atomic reduction: the plane's counts folded into the result, as ao_kernel's
// in_wave lanes write it.
__global__ void ao_finish_kernel(const AoArgs g, uint32_t width, uint32_t height, uint32_t xbound,
                                 const float4* __restrict__ feat, uint32_t* __restrict__ clear,
                                 float* __restrict__ ao, const uint32_t* __restrict__ plane,
                                 const unsigned long long* __restrict__ error_flag) {
  const bool err = *error_flag != 0ull;
  if (!err && g.in_wave) return;
  const uint64_t n_px = (uint64_t)width * height;
  for (uint64_t pix = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; pix < n_px;
       pix += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t px = (uint32_t)(pix % width);
    if (px >= xbound) {
      if (!g.in_wave) ao_store(g, kAoOutside, 0u, pix, clear, ao);
    } else if (err) {
      clear[pix] = 0xFFFFFFFFu;
      if (ao) ao[pix] = __builtin_nanf("");
    } else {
      ao_store(g, ao_classify(feat, pix), plane[pix], pix, clear, ao);
    }
  }
}

// First-hit feature buffers (zrt_ctx_features): one lane per pixel of the whole
// frame, lanes in 8x8 tiles as the render loops take them.  The pixel-centre
// primary ray (raytrace.zig:173-175 at r = 0.5: u = x / width, v = y / height;
// camera.zig:46-51), trace_kernel's closest hit, shade_step's hit record and
// albedo.  out: two float4 per pixel in the frame's layout, {N, t} and {A, id};
// id = the bits of uint32(prim + 1), prim the index in the reference's list.
template <int MODE, class StackT>
__global__ void __launch_bounds__(kBlock) features_kernel(const KArgs a, const uint32_t* __restrict__ slot_prim,
                                                          float4* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if ((MODE == 3 || MODE == 8) && !layout_ok(a)) return;
  if ((MODE == 3 || MODE == 8)) fill_lds_top(a, lds_top);
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t tiles_w = (a.width + 7u) / 8u;  // (tiles over the whole width here, not tiles_x)
  const uint32_t tile = gl >> 6, p = gl & 63u;
  const uint32_t px = (tile % tiles_w) * 8u + (p & 7u), py = (tile / tiles_w) * 8u + (p >> 3);
  if (px >= a.width || py >= a.height) return;
  float4* dst = out + 2ull * ((uint64_t)py * a.width + px);
  if (px >= a.xbound) {  // outside the rendered square (raytrace.zig:168)
    dst[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float u = (float)px / a.f_width;  // IEEE `/`
  const float v = (float)py / a.f_height;
  const V3 llc = mk(a.llc[0], a.llc[1], a.llc[2]);
  const V3 hor = mk(a.hor[0], a.hor[1], a.hor[2]);
  const V3 ver = mk(a.ver[0], a.ver[1], a.ver[2]);
  const V3 o = mk(a.org[0], a.org[1], a.org[2]);
  const V3 d = unit(sub(add(add(llc, scale(hor, u)), scale(ver, v)), o));
  float best_t;
  int best;
  closest_hit<MODE, StackT>(a, o, d, stk, lds_top, gl, best_t, best);
  if (best < 0) {
    const V3 bg = background(d);
    dst[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst[1] = make_float4(bg.x, bg.y, bg.z, 0.0f);
    return;
  }
  uint32_t c_shade = 0, c_tex = 0;
  Coh coh;
  HitRec h;
  hit_record<false, false>(a, a.mats, best, best_t, o, d, c_shade, c_tex, coh, h);
  const uint32_t code = h.mkind == ZRT_MAT_DIELECTRIC ? kAttOne : albedo_code<false>(h.mat, h.tag & 0x7fffffffu, h.tu, h.tv);
  const V3 alb = att_value<false>(a, a.mats, code);
  dst[0] = make_float4(h.normal.x, h.normal.y, h.normal.z, best_t);
  dst[1] = make_float4(alb.x, alb.y, alb.z, __uint_as_float(slot_prim[best] + 1u));
}

// A feature launch that set the device error flag (a traversal stack overflow)
// leaves NaN in the whole buffer, as a render launch does in its tiles.
__global__ void features_error_kernel(float4* __restrict__ out, uint64_t n_f4,
                                      const unsigned long long* __restrict__ error_flag) {
  if (*error_flag == 0ull) return;
  const float q = __builtin_nanf("");
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_f4; i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = make_float4(q, q, q, q);
}

// First-hit feature buffers along lens rays (zrt_ctx_camera_features): features_kernel's hit
// and outputs for the centre ray of a camera query's lens model, one lane per slot of the
// rectangle (camera_kernel's slots: 8 x 8 tiles anchored at (x0, y0)).  The centre ray is the
// query's sample ray at r1 = r2 = 0.5, where ((float)x + 0.5f) - 0.5f = (float)x exactly; the
// thin lens is taken at its centre.  g.kind is a kernel argument: the switch is a scalar branch.
// Pixels outside the rectangle are not touched.
template <int MODE, class StackT>
__global__ void __launch_bounds__(kBlock) lens_features_kernel(const KArgs a, const CameraArgs g,
                                                               const uint32_t* __restrict__ slot_prim,
                                                               float4* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;
  if (gl >= g.n) return;
  const uint32_t tile = gl >> 6, p = gl & 63u;
  const uint32_t ty = tile / g.tiles_w, tx = tile - ty * g.tiles_w;
  const uint32_t lx = tx * 8u + (p & 7u), ly = ty * 8u + (p >> 3);
  if (lx >= g.w || ly >= g.h) return;  // a slot outside the rectangle
  const uint32_t px = g.x0 + lx, py = g.y0 + ly;
  float4* dst = out + 2ull * ((uint64_t)py * g.width + px);
  const float u = (float)px / g.f_width;  // IEEE `/`, as features_kernel
  const float v = (float)py / g.f_height;
  const V3 org = mk(g.org[0], g.org[1], g.org[2]);
  const V3 aw = mk(g.aw[0], g.aw[1], g.aw[2]);
  V3 o = org, tgt;
  if (g.kind == ZRT_LENS_EQUIRECT) {
    float sp, cp, st, ct;
    dev::sincos_z(kTwoPi * u, &sp, &cp);
    dev::sincos_z(3.1415927f * v, &st, &ct);
    tgt = add(o, mk(st * cp, -ct, st * sp));
  } else if (g.kind == ZRT_LENS_FISHEYE) {
    const V3 au = mk(g.au[0], g.au[1], g.au[2]);
    const V3 av = mk(g.av[0], g.av[1], g.av[2]);
    const float qx = 2.0f * u - 1.0f, qy = 2.0f * v - 1.0f;
    const float r = dev::sqrt_rn(qx * qx + qy * qy);
    V3 dd = aw;
    if (r != 0.0f) {
      float sn, cs;
      dev::sincos_z(r * g.half_fov, &sn, &cs);
      const float k = dev::div_rn(sn, r);
      dd = add(add(scale(au, qx * k), scale(av, qy * k)), scale(aw, cs));
    }
    tgt = add(o, dd);
  } else {  // the view plane: Camera.getRay's point (camera.zig:47-49)
    const V3 llc = mk(g.llc[0], g.llc[1], g.llc[2]);
    const V3 hor = mk(g.hor[0], g.hor[1], g.hor[2]);
    const V3 ver = mk(g.ver[0], g.ver[1], g.ver[2]);
    const V3 P = add(add(llc, scale(hor, u)), scale(ver, v));
    if (g.kind == ZRT_LENS_ORTHO) {
      o = P;
      tgt = add(o, aw);
    } else {  // pinhole; the thin lens at its centre
      tgt = P;
    }
  }
  const V3 d = unit(sub(tgt, o));
  float best_t;
  int best;
  closest_hit<MODE, StackT>(a, o, d, stk, lds_top, gl, best_t, best);
  if (best < 0) {
    const V3 bg = background(d);
    dst[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dst[1] = make_float4(bg.x, bg.y, bg.z, 0.0f);
    return;
  }
  uint32_t c_shade = 0, c_tex = 0;
  Coh coh;
  HitRec h;
  hit_record<false, false>(a, a.mats, best, best_t, o, d, c_shade, c_tex, coh, h);
  const uint32_t code = h.mkind == ZRT_MAT_DIELECTRIC ? kAttOne : albedo_code<false>(h.mat, h.tag & 0x7fffffffu, h.tu, h.tv);
  const V3 alb = att_value<false>(a, a.mats, code);
  dst[0] = make_float4(h.normal.x, h.normal.y, h.normal.z, best_t);
  dst[1] = make_float4(alb.x, alb.y, alb.z, __uint_as_float(slot_prim[best] + 1u));
}

// Behind lens_features_kernel: a launch that set its error flag leaves NaN in the rectangle.
__global__ void lens_features_error_kernel(float4* __restrict__ out, const CameraArgs g,
                                           const unsigned long long* __restrict__ error_flag) {
  if (*error_flag == 0ull) return;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  const uint32_t tile = i >> 6, l = i & 63u;
  const uint32_t ty = tile / g.tiles_w, tx = tile - ty * g.tiles_w;
  const uint32_t lx = tx * 8u + (l & 7u), ly = ty * 8u + (l >> 3);
  if (lx >= g.w || ly >= g.h) return;
  const float q = __builtin_nanf("");
  float4* dst = out + 2ull * ((uint64_t)(g.y0 + ly) * g.width + (g.x0 + lx));
  dst[0] = make_float4(q, q, q, q);
  dst[1] = make_float4(q, q, q, q);
}

// Per-pixel sum of the chunk sums in chunk order, times 1/spp
// (raytrace.zig:182), into the rank's tile-major output.  A launch that set the
// device error flag (a traversal stack overflow) leaves NaN in every pixel, so
// a caller that never asks for the status still cannot take the frame for a
// correct one (the status itself: zrt_ctx_sync / zrt_ctx_stats / zrt_render).
__global__ void finalize_kernel(const float4* __restrict__ partial, float* __restrict__ out,
                                uint32_t n_slots, uint32_t n_chunks, uint32_t world, uint32_t rank,
                                uint32_t tiles_x, uint32_t xbound, uint32_t height, float color_scale,
                                const unsigned long long* __restrict__ error_flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t lt = i >> 6, p = i & 63u;
  const uint32_t t = lt * world + rank;
  const uint32_t px = (t % tiles_x) * 8u + (p & 7u);
  const uint32_t py = (t / tiles_x) * 8u + (p >> 3);
  float r = 0.0f, g = 0.0f, b = 0.0f;
  if (*error_flag != 0ull) {
    r = g = b = __builtin_nanf("");
  } else if (px < xbound && py < height) {
    for (uint32_t j = 0; j < n_chunks; ++j) {  // [chunk][slot]: a wave reads 1 KiB per chunk
      const float4 v = partial[(size_t)j * n_slots + i];
      r += v.x;
      g += v.y;
      b += v.z;
    }
    r *= color_scale;
    g *= color_scale;
    b *= color_scale;
  }
  out[3ull * i + 0] = r;
  out[3ull * i + 1] = g;
  out[3ull * i + 2] = b;
}

// png_image.zig:136-138 on the device (image_io.cpp png_channel): std.math.min / max
// are `x < y ? x : y` / `x > y ? x : y`, clamp = max(lower, min(val, upper))
__device__ __forceinline__ uint32_t png_channel_dev(float c) {
  const float v = 255.999f * c;
  const float m = v < 255.0f ? v : 255.0f;
  return uint32_t(0.0f > m ? 0.0f : m);
}

// finalize_kernel's progressive counterpart (zrt_ctx_accum_pass): a pass's chunk
// sums added, in chunk order, onto the run's resident per-slot sums, which are
// stored back; the frame written is the sum times new_scale = 1 / (samples in
// the accumulator after the pass) - the bits finalize_kernel gives for a whole
// frame of that many samples (raytrace.zig:157, 177, 182).  Out-of-frame slots
// stay 0.  A nonzero device error flag leaves NaN in every pixel and in every
// slot of accum, so no later pass resolves a clean frame from it.
// accum[i].w is Q, the second moment of the slot's chunk sums (zrt.h "the variance
// plane"): per chunk sum S_j of the first q_chunks of the pass (all of them but a
// ragged last one), l = (S_j.r + S_j.g) + S_j.b, Q = Q + l * l, in chunk order.
// metrics: kMetricShards pairs, kMetricStride words apart (a block adds into pair
// blockIdx.x % kMetricShards: one word takes some 90 atomics per microsecond, and a
// 2048 x 2048 frame has 65 536 waves; the host adds the pairs up).  Word 0: in-frame
// pixels whose 8-bit PNG value (any channel) differs between this frame and the one
// shown before the pass (accum before x prev_scale; prev_scale is 0 before the first
// pass); word 1: the bits of the largest |new - previous| over the in-frame channels
// (non-negative floats order as their bit patterns; a NaN difference is skipped).
// At most one atomic of each per wave (none for a maximum already reached: the word
// only grows, so a stale read can only cost an atomic, never skip one).
__global__ void accumulate_kernel(const float4* __restrict__ partial, float4* __restrict__ accum,
                                  float* __restrict__ out, uint32_t n_slots, uint32_t pass_chunks, uint32_t world,
                                  uint32_t rank, uint32_t tiles_x, uint32_t xbound, uint32_t height, float prev_scale,
                                  float new_scale, uint32_t q_chunks, const unsigned long long* __restrict__ error_flag,
                                  unsigned long long* __restrict__ metrics) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n_slots;
  const uint32_t lt = i >> 6, p = i & 63u;
  const uint32_t t = lt * world + rank;
  const uint32_t px = (t % tiles_x) * 8u + (p & 7u);
  const uint32_t py = (t / tiles_x) * 8u + (p >> 3);
  float r = 0.0f, g = 0.0f, b = 0.0f;
  float change = 0.0f;
  bool changed = false;
  if (live && *error_flag != 0ull) {
    r = g = b = __builtin_nanf("");
    accum[i] = make_float4(r, g, b, r);
  } else if (live && px < xbound && py < height) {
    const float4 before = accum[i];
    r = before.x;
    g = before.y;
    b = before.z;
    float q = before.w;
    for (uint32_t j = 0; j < pass_chunks; ++j) {  // [chunk][slot], as finalize_kernel reads them
      const float4 v = partial[(size_t)j * n_slots + i];
      r += v.x;
      g += v.y;
      b += v.z;
      if (j < q_chunks) {  // (a ragged last chunk is left out of the second moment)
        const float l = (v.x + v.y) + v.z;
        q = q + l * l;
      }
    }
    accum[i] = make_float4(r, g, b, q);
    r *= new_scale;
    g *= new_scale;
    b *= new_scale;
    const float pr = before.x * prev_scale, pg = before.y * prev_scale, pb = before.z * prev_scale;
    const float dr = fabsf(r - pr), dg = fabsf(g - pg), db = fabsf(b - pb);
    change = dr > change ? dr : change;  // (a NaN compares false: skipped)
    change = dg > change ? dg : change;
    change = db > change ? db : change;
    changed = png_channel_dev(r) != png_channel_dev(pr) || png_channel_dev(g) != png_channel_dev(pg) ||
              png_channel_dev(b) != png_channel_dev(pb);
  }
  if (live) {
    out[3ull * i + 0] = r;
    out[3ull * i + 1] = g;
    out[3ull * i + 2] = b;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(change, off, 64);
    change = o > change ? o : change;
  }
  const unsigned long long ballot = __ballot(changed);
  if ((threadIdx.x & 63u) == 0u) {
    unsigned long long* m = metrics + (blockIdx.x % kMetricShards) * kMetricStride;
    if (ballot) atomicAdd(&m[0], (unsigned long long)__popcll(ballot));
    unsigned int* mx = reinterpret_cast<unsigned int*>(&m[1]);
    const unsigned int bits = __float_as_uint(change);
    if (bits > __hip_atomic_load(mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mx, bits);
  }
}

// accumulate_kernel for a level of an adaptive run (zrt_ctx_adapt_level; the rule:
// zrt.h "adaptive sampling"): one wave per ACTIVE tile (wave w takes tile active[w]),
// lane = pixel.  The level's chunk sums are added onto accum in chunk order and the
// tile's preview (sum x new_scale) is written to out, as accumulate_kernel does; the
// sums read before the add are the previous level's, so H = before x prev_scale is the
// preview at L_(k-1) with no second buffer: accum is the snapshot.  decide: lanes
// failing d <= tolerance * sqrtf(s) are balloted and a tile without one is frozen.
// tile_done[lt] = the tile's samples per pixel (level_samples), bit 31 set once frozen.
// metrics as accumulate_kernel's, over the tiles touched, plus word 2 of each pair's
// shard: in-frame pixels resolved.  A nonzero error flag: the waves stride over ALL
// the rank's tiles, leave NaN in accum and out and freeze them (nothing survives).
__global__ void resolve_kernel(const float4* __restrict__ partial, float4* __restrict__ accum,
                               float* __restrict__ out, const uint32_t* __restrict__ active, uint32_t n_active,
                               uint32_t my_tiles, uint32_t pass_chunks, uint32_t world, uint32_t rank,
                               uint32_t tiles_x, uint32_t xbound, uint32_t height, float prev_scale, float new_scale,
                               uint32_t q_chunks, float tolerance, uint32_t decide, uint32_t level_samples,
                               uint32_t* __restrict__ tile_done, const unsigned long long* __restrict__ error_flag,
                               unsigned long long* __restrict__ metrics) {
  const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, p = threadIdx.x & 63u;
  if (w >= n_active) return;  // (whole waves)
  const size_t n_slots = size_t(my_tiles) * 64u;
  if (*error_flag != 0ull) {
    const float nan = __builtin_nanf("");
    for (uint32_t lt = w; lt < my_tiles; lt += n_active) {
      const size_t i = size_t(lt) * 64u + p;
      accum[i] = make_float4(nan, nan, nan, nan);
      out[3ull * i + 0] = nan;
      out[3ull * i + 1] = nan;
      out[3ull * i + 2] = nan;
      if (p == 0u) tile_done[lt] |= kTileFrozen;
    }
    return;
  }
  const uint32_t lt = active[w];
  const size_t i = size_t(lt) * 64u + p;
  const uint32_t t = lt * world + rank;
  const uint32_t px = (t % tiles_x) * 8u + (p & 7u);
  const uint32_t py = (t / tiles_x) * 8u + (p >> 3);
  const bool in_frame = px < xbound && py < height;
  float r = 0.0f, g = 0.0f, b = 0.0f;
  float change = 0.0f;
  bool changed = false, failing = false;
  if (in_frame) {
    const float4 before = accum[i];
    r = before.x;
    g = before.y;
    b = before.z;
    float q = before.w;
    for (uint32_t j = 0; j < pass_chunks; ++j) {  // [chunk][slot] over all the rank's slots
      const float4 v = partial[(size_t)j * n_slots + i];
      r += v.x;
      g += v.y;
      b += v.z;
      if (j < q_chunks) {  // (as accumulate_kernel)
        const float l = (v.x + v.y) + v.z;
        q = q + l * l;
      }
    }
    accum[i] = make_float4(r, g, b, q);
    r *= new_scale;
    g *= new_scale;
    b *= new_scale;
    const float pr = before.x * prev_scale, pg = before.y * prev_scale, pb = before.z * prev_scale;
    const float dr = fabsf(r - pr), dg = fabsf(g - pg), db = fabsf(b - pb);
    change = dr > change ? dr : change;  // (a NaN compares false: skipped)
    change = dg > change ? dg : change;
    change = db > change ? db : change;
    changed = png_channel_dev(r) != png_channel_dev(pr) || png_channel_dev(g) != png_channel_dev(pg) ||
              png_channel_dev(b) != png_channel_dev(pb);
    const float d = (dr + dg) + db;
    const float s = (r + g) + b;
    failing = !(d <= tolerance * __builtin_sqrtf(s));  // (HIP's IEEE sqrtf; a NaN anywhere: the lane fails)
  }
  out[3ull * i + 0] = r;
  out[3ull * i + 1] = g;
  out[3ull * i + 2] = b;
  for (int off = 32; off > 0; off >>= 1) {
    const float o = __shfl_xor(change, off, 64);
    change = o > change ? o : change;
  }
  const unsigned long long ballot = __ballot(changed), fails = __ballot(failing), inside = __ballot(in_frame);
  if (p == 0u) {
    tile_done[lt] = level_samples | (decide && fails == 0ull ? kTileFrozen : 0u);
    unsigned long long* m = metrics + (blockIdx.x % kMetricShards) * kMetricStride;
    if (ballot) atomicAdd(&m[0], (unsigned long long)__popcll(ballot));
    if (inside) atomicAdd(&m[2], (unsigned long long)__popcll(inside));
    unsigned int* mx = reinterpret_cast<unsigned int*>(&m[1]);
    const unsigned int bits = __float_as_uint(change);
    if (bits > __hip_atomic_load(mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(mx, bits);
  }
}

// The tiles of `in` that resolve_kernel left unfrozen, packed into `out` in their
// order (so the probe's costliest-first order survives a level), and their number.
// One block: per round of blockDim.x list entries a ballot and the lanes' mbcnt ranks
// within each wave, the waves' counts scanned through LDS, a running base across rounds.
// out[base + ...] stays below the number of entries read, so within n.
// (One body for both predicates, as text: as a template over the predicate the first
// kernel's sums came out reassociated, and it is compared with its earlier assembly.)
constexpr uint32_t kCompactBlock = 1024;
#define ZRT_COMPACT_BODY(KEEP)                                                                                      \
  __shared__ uint32_t wave_count[kCompactBlock / 64];                                                               \
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;                                                   \
  uint32_t base = 0;                                                                                                \
  for (uint32_t start = 0; start < n; start += kCompactBlock) {                                                     \
    const uint32_t pos = start + threadIdx.x;                                                                       \
    uint32_t lt = 0;                                                                                                \
    bool keep = false;                                                                                              \
    if (pos < n) {                                                                                                  \
      lt = in[pos];                                                                                                 \
      keep = KEEP;                                                                                                  \
    }                                                                                                               \
    const unsigned long long b = __ballot(keep);                                                                    \
    const uint32_t below = __builtin_amdgcn_mbcnt_hi(uint32_t(b >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(b), 0u)); \
    if (lane == 0u) wave_count[wv] = uint32_t(__popcll(b));                                                         \
    __syncthreads();                                                                                                \
    uint32_t off = 0, total = 0;                                                                                    \
    for (uint32_t k = 0; k < kCompactBlock / 64; ++k) {                                                             \
      const uint32_t v = wave_count[k];                                                                             \
      off += k < wv ? v : 0u;                                                                                       \
      total += v;                                                                                                   \
    }                                                                                                               \
    if (keep) out[base + off + below] = lt;                                                                         \
    base += total;                                                                                                  \
    __syncthreads();                                                                                                \
  }                                                                                                                 \
  if (threadIdx.x == 0u) *count = base;
__global__ void __launch_bounds__(kCompactBlock) compact_kernel(const uint32_t* __restrict__ in, uint32_t n,
                                                                const uint32_t* __restrict__ tile_done,
                                                                uint32_t* __restrict__ out,
                                                                uint32_t* __restrict__ count) {
  ZRT_COMPACT_BODY((tile_done[lt] & kTileFrozen) == 0u)
}
// ... and the tiles whose class word is `word` (the general and the one-sphere tiles of a
// classified frame, each in the probe's order)
__global__ void __launch_bounds__(kCompactBlock) compact_class_kernel(const uint32_t* __restrict__ in, uint32_t n,
                                                                      const uint32_t* __restrict__ cls, uint32_t word,
                                                                      uint32_t* __restrict__ out,
                                                                      uint32_t* __restrict__ count) {
  ZRT_COMPACT_BODY(cls[lt] == word)
}
#undef ZRT_COMPACT_BODY

// Scatter gathered rank tiles into the framebuffer (raytrace.zig:182 layout).
// Packed (stride_px == 0): rank r's tiles start at rank_base[r].  Padded: rank r
// starts at r * stride_px, as a gather of equal per-rank counts leaves them.
// CH: floats per pixel, 3 (the frame) or 1 (a plane, zrt_ctx_assemble_plane).
template <uint32_t CH>
__global__ void assemble_kernel(const float* __restrict__ gathered, float* __restrict__ frame,
                                const uint32_t* __restrict__ rank_base, uint32_t world,
                                uint32_t tiles_x, uint32_t xbound, uint32_t height, uint32_t width,
                                uint32_t total, uint32_t stride_px, uint32_t n_tiles) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  uint32_t r = 0, w = 0;
  if (stride_px) {
    r = i / stride_px;
    w = i - r * stride_px;
  } else {
    // find the rank owning gathered pixel i (world is small)
    while (r + 1 < world && rank_base[r + 1] <= i) ++r;
    w = i - rank_base[r];
  }
  const uint32_t lt = w >> 6, p = w & 63u;
  const uint32_t t = lt * world + r;
  if (t >= n_tiles) return;  // padding
  const uint32_t px = (t % tiles_x) * 8u + (p & 7u);
  const uint32_t py = (t / tiles_x) * 8u + (p >> 3);
  if (px >= xbound || py >= height) return;
  const size_t o = ((size_t)py * width + px) * CH;
#pragma unroll
  for (uint32_t c = 0; c < CH; ++c) frame[o + c] = gathered[(size_t)CH * i + c];
}

// The variance plane of a run (zrt_ctx_accum_variance; the definition: zrt.h "the variance
// plane"): per in-frame slot, from the accumulator's sums and second moment Q and the
// tile's host-computed {ik, sc} (plan_variance), in f32, nothing fused:
// mean = M ik, v = Q ik - mean mean clamped at 0 (a NaN stays), var = v sc.
// Out-of-frame slots are 0; a nonzero device error flag leaves NaN in every slot.
__global__ void variance_kernel(const float4* __restrict__ accum, const float2* __restrict__ tile_plan,
                                float* __restrict__ out, uint32_t n_slots, uint32_t world, uint32_t rank,
                                uint32_t tiles_x, uint32_t xbound, uint32_t height,
                                const unsigned long long* __restrict__ error_flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_slots) return;
  const uint32_t lt = i >> 6, p = i & 63u;
  const uint32_t t = lt * world + rank;
  const uint32_t px = (t % tiles_x) * 8u + (p & 7u);
  const uint32_t py = (t / tiles_x) * 8u + (p >> 3);
  float var = 0.0f;
  if (*error_flag != 0ull) {
    var = __builtin_nanf("");
  } else if (px < xbound && py < height) {
    const float4 a = accum[i];
    const float2 k = tile_plan[lt];
    const float m = (a.x + a.y) + a.z;
    const float mean = m * k.x;
    float v = a.w * k.x - mean * mean;
    v = (v > 0.0f || v != v) ? v : 0.0f;
    var = v * k.y;
  }
  out[i] = var;
}

// Device evaluation of the path's math (parity probes against the oracle).
__global__ void debug_math_kernel(int fn, const float* __restrict__ x, const float* __restrict__ y,
                                  float* __restrict__ out, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = x[i], b = y ? y[i] : 0.0f;
  float s, c, r;
  switch (fn) {
    case 0: dev::sincos_z(a, &s, &c); r = s; break;
    case 1: dev::sincos_z(a, &s, &c); r = c; break;
    case 2: r = dev::acos_z(a); break;
    case 3: r = dev::atan_z(a); break;
    case 4: r = dev::sqrt_rn(a); break;
    case 5: r = dev::atan2_z(a, b); break;
    case 6: r = dev::pow5_z(a); break;
    case 8: r = dev::rcp_rn(a); break;
    case 9: r = dev::div_rn(a, b); break;
    default: r = a / b; break;
  }
  out[i] = r;
}

// Self-check of the short correctly rounded divisions (device_math.hpp) against
// HIP's IEEE `/` and sqrtf on this device: counts[0] rcp_rn and sqrt_rn over all
// 2^32 inputs; [1] div_rn
// over n hashed pairs (every exponent, signed zeros, subnormals, inf, NaN, and
// dividends near short multiples of the divisor); [2] unit() over n vectors (wide
// exponents, zero / tiny components); [3] inv_dir over n triples; [4] the jitter
// quotient (x + r - 0.5) / width with y = RN(1/width) over n (width, x, r) draws.
__device__ __forceinline__ uint32_t mix32(uint64_t x) {
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return uint32_t(x);
}
__device__ __forceinline__ bool same_f(float x, float y) {
  return __float_as_uint(x) == __float_as_uint(y) || (x != x && y != y);
}
__device__ __forceinline__ float wild_float(uint32_t h, uint32_t h2) {  // any class, biased to edges
  switch (h2 & 15) {
    case 0: return __uint_as_float(h & 0x807fffffu);                       // +-0, subnormal
    case 1: return __uint_as_float((h & 0x807fffffu) | 0x7f800000u);        // +-inf, NaN
    case 2: return __uint_as_float((h & 0x80ffffffu) | (((h2 >> 4) & 3u) << 23) | 0x3f000000u);  // near 1
    default: return __uint_as_float(h);                                     // any pattern
  }
}
__global__ void debug_division_kernel(uint64_t n, unsigned long long* __restrict__ counts) {
  const uint64_t tid = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
  const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
  uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
  for (uint64_t i = tid; i < (1ull << 32); i += stride) {
    const float b = __uint_as_float(uint32_t(i));
    c0 += same_f(dev::rcp_rn(b), 1.0f / b) ? 0u : 1u;
    c0 += same_f(dev::sqrt_rn(b), __builtin_sqrtf(b)) ? 0u : 1u;
  }
  for (uint64_t i = tid; i < n; i += stride) {
    const uint32_t h0 = mix32(8 * i), h1 = mix32(8 * i + 1), h2 = mix32(8 * i + 2), h3 = mix32(8 * i + 3);
    const uint32_t h4 = mix32(8 * i + 4), h5 = mix32(8 * i + 5);
    // [1] div_rn
    float a = wild_float(h0, h2), b = wild_float(h1, h2 >> 8);
    if ((h3 & 3) == 0) {  // a close to a short multiple of b (quotients near rounding midpoints)
      const float k = float(int(h3 >> 20) + 1) * 0.0009765625f;
      a = __uint_as_float(__float_as_uint(b * k) + int((h3 >> 2) & 7) - 3);
    }
    c1 += same_f(dev::div_rn(a, b), a / b) ? 0u : 1u;
    // [2] unit(): components of one vector share an exponent window, some zero / tiny
    const int e0 = int(h4 & 255) - 128;
    V3 v;
    float* vp = &v.x;
    for (int k = 0; k < 3; ++k) {
      const uint32_t hk = mix32(8 * i + 6 + uint64_t(k) * 0x100000000ull);
      const int e = e0 + int((hk >> 24) & 31) - 16;
      const uint32_t bexp = uint32_t(e + 127 < 1 ? 0 : e + 127 > 254 ? 254 : e + 127);
      float x = __uint_as_float((hk & 0x807fffffu) | (bexp << 23));
      if (((h5 >> (4 * k)) & 15) == 0) x = (hk & 1) ? -0.0f : 0.0f;
      if (((h5 >> (4 * k)) & 15) == 1) x = __uint_as_float(hk & 0x800fffffu);  // subnormal
      vp[k] = x;
    }
    const float l = __builtin_sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
    const V3 u = unit(v);
    c2 += (same_f(u.x, v.x / l) && same_f(u.y, v.y / l) && same_f(u.z, v.z / l) && same_f(unit_y(v), v.y / l)) ? 0u : 1u;
    // [3] inv_dir over the same triples and over unit directions
    float ix, iy, iz;
    inv_dir(v.x, v.y, v.z, ix, iy, iz);
    c3 += (same_f(ix, 1.0f / v.x) && same_f(iy, 1.0f / v.y) && same_f(iz, 1.0f / v.z)) ? 0u : 1u;
    inv_dir(u.x, u.y, u.z, ix, iy, iz);
    c3 += (same_f(ix, 1.0f / u.x) && same_f(iy, 1.0f / u.y) && same_f(iz, 1.0f / u.z)) ? 0u : 1u;
    // [4] jitter (raytrace.zig:173): width in [1, 65535], x < 65536, r = Random.float
    const float w = float((h0 & 0xffffu) | 1u) + float((h1 >> 16) & 0xfffeu);
    const float fw = w > 65535.0f ? 65535.0f : w;
    const float px = float(h2 & 0xffffu) * ((h3 >> 30) ? 1.0f : 0.0f);  // many x = 0 (tiny quotients)
    const float r = __uint_as_float((0x7fu << 23) | (h4 >> 9)) - 1.0f;
    const float num = px + r - 0.5f;
    c4 += same_f(dev::div_core(num, fw, 1.0f / fw), num / fw) ? 0u : 1u;
  }
  if (c0) atomicAdd(&counts[0], (unsigned long long)c0);
  if (c1) atomicAdd(&counts[1], (unsigned long long)c1);
  if (c2) atomicAdd(&counts[2], (unsigned long long)c2);
  if (c3) atomicAdd(&counts[3], (unsigned long long)c3);
  if (c4) atomicAdd(&counts[4], (unsigned long long)c4);
}

template <int PRNG>
__global__ void debug_rng_kernel(uint64_t key, unsigned long long* out, uint32_t n) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  Rng<PRNG> r;
  r.init(key);
  for (uint32_t i = 0; i < n; ++i) out[i] = r.next();
}

// ---------------------------------------------------------------------------
// Radiance queries (zrt_ctx_radiance; zrt.h "radiance queries"): rayColor
// along caller-supplied rays.  render_loop's sampling loop with its primary ray read from
// a buffer instead of built by Camera.getRay: the sample's stream is keyed by (ray index,
// sample), the two jitter floats are drawn and dropped, and each loop trip is one rayColor
// step - trace_kernel's closest hit (so any origin and any direction are served as there),
// then shade_step; a path that ends in the sky takes att_product over its rows.
// A work item is one (ray, chunk) and a lane runs its item's samples on its own, the
// chunk's sequential sum in registers.  Within a round item k is ray k % n of chunk k / n.
// The grid is bounded (zrt::plan_radiance): a block loops over its items, block b taking
// items b * 256 + 256 * grid * t, and its lanes keep one stack column and one column of
// attenuation rows each (gl) however many rays the call has.  A wave's first item is
// wave-uniform, so the one 64-bit division is scalar.  The chunk sums are parked in
// [chunk][ray]; radiance_finish_kernel folds them.  No lane state is parked in LDS across
// the traversal: the wave is not in lockstep, and closest_hit takes the ray by value.
// FAST is built for 4 waves per SIMD (128 VGPRs), ao_kernel's occupancy: left to itself the
// compiler takes 122 (xoroshiro) / 130 (xoshiro) and the latter drops to 3.
// ---------------------------------------------------------------------------
template <int MODE, int PRNG, class StackT>
__global__ void __launch_bounds__(kBlock, MODE == 3 ? 4 : 1) radiance_kernel(const KArgs a, const RadianceArgs g,
                                                                             const float* __restrict__ rays) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  lds_u32* att_l = (lds_u32*)(lds_raw + a.lds_att_off) + threadIdx.x;  // [row][lane] att codes
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const DevMaterial* mats = a.mats;
  if (a.mats_in_lds) {  // block-uniform
    float4* m = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
    fill_lds_mats(a, m);
    mats = reinterpret_cast<const DevMaterial*>(m);
  }
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;  // n_lanes < 2^32
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const AttRows ar{att_l, kBlock, gl, a.n_lanes};
  uint32_t c_refl = 0, c_bg = 0, c_depth = 0, c_shade = 0, c_tex = 0;
  uint32_t deepest = 0;  // the most attenuation rows a path of this lane pushed (kRqDeepestSlot)
  Coh coh;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < g.n_items; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i0 = base + wave * 64u;  // the wave's first item
    const uint64_t c0 = i0 / g.n;
    const uint64_t k = (i0 - c0 * g.n) + lane;  // < n + 64
    const uint32_t dq = g.n >= 64u ? (k >= g.n ? 1u : 0u) : (uint32_t)k / g.n;
    const uint32_t ray = (uint32_t)(k - (uint64_t)dq * g.n);
    const uint64_t cj = c0 + dq;  // the item's chunk within the round
    if (cj * g.n + ray >= g.n_items) continue;  // past the round's end
    const uint32_t s_end = min(g.sample0 + ((uint32_t)cj + 1u) * g.chunk, g.sample_end);
    uint32_t sample = g.sample0 + (uint32_t)cj * g.chunk;
    const float* q = rays + 6ull * ray;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    uint32_t depth_left = 0;
    bool in_sample = false;
    Rng<PRNG> rng;
    rng.init(0);
    for (;;) {
      if (!in_sample) {  // a new sample: its stream, the dropped jitter, Ray.init (ray.zig:11-13)
        rng.init((((uint64_t)ray << 16) | (uint64_t)sample) + g.key_offset);
        (void)rand_float(rng);
        (void)rand_float(rng);
        o = mk(q[0], q[1], q[2]);
        d = unit(mk(q[3], q[4], q[5]));
        depth_left = a.max_depth;
        in_sample = true;
      }
      // ---- one rayColor step (raytrace.zig:62-100)
      bool path_end = false, sky = false;
      V3 L = mk(0.0f, 0.0f, 0.0f);
      if (depth_left == 0) {
        ++c_depth;
        path_end = true;
      } else {
        float best_t;
        int best;
        closest_hit<MODE, StackT>(a, o, d, stk, lds_top, gl, best_t, best);
        shade_step<false, Rng<PRNG>>(a, mats, ar, rng, best, best_t, o, d, depth_left, path_end, sky, L, c_bg, c_refl,
                                     c_shade, c_tex, coh);
      }
      if (path_end) {
        const V3 col = sky ? att_product<false>(a, mats, ar, a.max_depth - depth_left, L, coh) : L;
        acc_r += col.x;
        acc_g += col.y;
        acc_b += col.z;
        // (shade_step pushes a scatter's row while depth_left > 1: the one at depth 1 is never read)
        deepest = max(deepest, a.max_depth - depth_left - (depth_left == 0 && a.max_depth != 0 ? 1u : 0u));
        in_sample = false;
        if (++sample == s_end) break;  // the chunk's sequential sum is complete
      }
    }
    a.partial[cj * g.n + ray] = make_float4(acc_r, acc_g, acc_b, 0.0f);
  }
  wave_add_u64(&a.counters[kDepthHits], c_depth);
  wave_add_u64(&a.counters[kReflections], c_refl);
  wave_add_u64(&a.counters[kBackground], c_bg);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) deepest = max(deepest, (uint32_t)__shfl_xor((int)deepest, off));
  if (lane == 0 && deepest) atomicMax(&a.counters[kRqDeepestSlot], (unsigned long long)deepest);
}

// Behind radiance_kernel, one lane per ray: the round's n_chunks parked sums added onto
// the ray's sum in chunk order (started from 0 where zero_first), each add rounded once.
// final (after the call's last round): rgb = sum * scale (raytrace.zig:157, 182), or, after
// a launch that set its error flag (a traversal stack overflow), NaN in sum.rgb and rgb.
__global__ void radiance_finish_kernel(const float4* __restrict__ partial, uint32_t n, uint32_t n_chunks,
                                       uint32_t zero_first, float4* __restrict__ sum, float* __restrict__ rgb,
                                       float scale, uint32_t final,
                                       const unsigned long long* __restrict__ error_flag) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 s = zero_first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : sum[i];
  for (uint32_t j = 0; j < n_chunks; ++j) {
    const float4 p = partial[(uint64_t)j * n + i];
    s.x += p.x;
    s.y += p.y;
    s.z += p.z;
  }
  if (final && *error_flag != 0ull) s.x = s.y = s.z = __builtin_nanf("");
  sum[i] = make_float4(s.x, s.y, s.z, 0.0f);
  if (final && rgb) {
    rgb[3ull * i + 0] = s.x * scale;
    rgb[3ull * i + 1] = s.y * scale;
    rgb[3ull * i + 2] = s.z * scale;
  }
}

// ---------------------------------------------------------------------------
// Camera queries (zrt_ctx_camera; zrt.h "camera queries"): frames through
// device-generated lens rays.  radiance_kernel's item loop with the primary ray generated
// at each sample start instead of read from a buffer: the sample's stream is the render's
// own (keyed by the pixel's frame offset and the sample), its two jitter floats are used,
// and a lens model (g.kind: a kernel argument, so the switch is a scalar branch and the
// descriptor stays in SGPRs) maps (u, v) to an origin and a target; dir = tgt - o.  A model
// that samples its lens draws from the stream of key ^ kLensStream through the same
// generator object before the sample's stream is started.
// A work item is one (slot, chunk).  Slots enumerate the rectangle in 8 x 8 tiles anchored
// at (x0, y0), 64 slots per tile, so g.n is a multiple of 64: a wave's 64 items are one tile
// of one chunk (the render's primary-ray coherence) and the one 64-bit division is scalar.
// Slots outside the rectangle do no work and park nothing; camera_finish_kernel reads only
// the slots inside.  Everything else - the bounded grid, the rows per lane of the grid,
// [chunk][slot] parked sums, the counters, FAST's 4 waves per SIMD - is radiance_kernel's.
// ---------------------------------------------------------------------------
constexpr uint64_t kLensStream = 0xD1B54A32D192ED03ULL;

template <int MODE, int PRNG, class StackT>
__global__ void __launch_bounds__(kBlock, MODE == 3 ? 4 : 1) camera_kernel(const KArgs a, const CameraArgs g) {
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];
  StackT* stk = reinterpret_cast<StackT*>(lds_raw) + threadIdx.x;
  float4* lds_top = reinterpret_cast<float4*>(lds_raw + a.lds_top_off);
  lds_u32* att_l = (lds_u32*)(lds_raw + a.lds_att_off) + threadIdx.x;  // [row][lane] att codes
  if (MODE == 3 && !layout_ok(a)) return;
  if (MODE == 3) fill_lds_top(a, lds_top);
  const DevMaterial* mats = a.mats;
  if (a.mats_in_lds) {  // block-uniform
    float4* m = reinterpret_cast<float4*>(lds_raw + a.lds_mat_off);
    fill_lds_mats(a, m);
    mats = reinterpret_cast<const DevMaterial*>(m);
  }
  const uint32_t gl = blockIdx.x * kBlock + threadIdx.x;  // n_lanes < 2^32
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const AttRows ar{att_l, kBlock, gl, a.n_lanes};
  uint32_t c_refl = 0, c_bg = 0, c_depth = 0, c_shade = 0, c_tex = 0;
  uint32_t deepest = 0;  // the most attenuation rows a path of this lane pushed (kRqDeepestSlot)
  Coh coh;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < g.n_items; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i0 = base + wave * 64u;  // the wave's first item: slot 0 of a tile
    if (i0 >= g.n_items) continue;          // past the round's end (n_items is a multiple of 64)
    const uint64_t cj = i0 / g.n;           // the wave's chunk within the round
    const uint32_t slot0 = (uint32_t)(i0 - cj * g.n);
    const uint32_t tile = slot0 >> 6;
    const uint32_t ty = tile / g.tiles_w, tx = tile - ty * g.tiles_w;
    const uint32_t lx = tx * 8u + (lane & 7u), ly = ty * 8u + (lane >> 3);
    if (lx >= g.w || ly >= g.h) continue;  // a slot outside the rectangle
    const uint32_t px = g.x0 + lx, py = g.y0 + ly;
    const uint64_t pixel_key = (((uint64_t)py * g.width + px) << 16) + g.key_offset;  // (the sample field is free)
    const float fx = (float)px, fy = (float)py;
    const uint32_t s_end = min(g.sample0 + ((uint32_t)cj + 1u) * g.chunk, g.sample_end);
    uint32_t sample = g.sample0 + (uint32_t)cj * g.chunk;
    float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
    V3 o = mk(0.0f, 0.0f, 0.0f), d = mk(0.0f, 0.0f, 1.0f);
    uint32_t depth_left = 0;
    bool in_sample = false;
    Rng<PRNG> rng;
    rng.init(0);
    for (;;) {
      if (!in_sample) {  // a new sample: lens floats, its stream, jitter, the model, Ray.init (ray.zig:11-13)
        // (R << 16 has its low 16 bits clear and sample < 65536: the sum is the `|` of the definition)
        const uint64_t key = pixel_key + (uint64_t)sample;
        float la = 0.0f, lb = 0.0f;
        if (g.kind == ZRT_LENS_THIN) {  // a point of the unit disc by rejection, on the lens stream
          rng.init(key ^ kLensStream);
          do {
            la = 2.0f * rand_float(rng) - 1.0f;
            lb = 2.0f * rand_float(rng) - 1.0f;
          } while (!(la * la + lb * lb < 1.0f));
        }
        rng.init(key);
        const float r1 = rand_float(rng);
        const float r2 = rand_float(rng);
        const float u = dev::div_rn((fx + r1) - 0.5f, g.f_width);  // raytrace.zig:173-174
        const float v = dev::div_rn((fy + r2) - 0.5f, g.f_height);
        const V3 org = mk(g.org[0], g.org[1], g.org[2]);
        const V3 au = mk(g.au[0], g.au[1], g.au[2]);
        const V3 av = mk(g.av[0], g.av[1], g.av[2]);
        const V3 aw = mk(g.aw[0], g.aw[1], g.aw[2]);
        V3 tgt;
        if (g.kind == ZRT_LENS_EQUIRECT) {
          float sp, cp, st, ct;
          dev::sincos_z(kTwoPi * u, &sp, &cp);
          dev::sincos_z(3.1415927f * v, &st, &ct);
          o = org;
          tgt = add(o, mk(st * cp, -ct, st * sp));
        } else if (g.kind == ZRT_LENS_FISHEYE) {
          const float qx = 2.0f * u - 1.0f, qy = 2.0f * v - 1.0f;
          const float r = dev::sqrt_rn(qx * qx + qy * qy);
          V3 dd = aw;
          if (r != 0.0f) {
            float sn, cs;
            dev::sincos_z(r * g.half_fov, &sn, &cs);
            const float k = dev::div_rn(sn, r);
            dd = add(add(scale(au, qx * k), scale(av, qy * k)), scale(aw, cs));
          }
          o = org;
          tgt = add(o, dd);
        } else {  // the view plane: Camera.getRay's point (camera.zig:47-49)
          const V3 llc = mk(g.llc[0], g.llc[1], g.llc[2]);
          const V3 hor = mk(g.hor[0], g.hor[1], g.hor[2]);
          const V3 ver = mk(g.ver[0], g.ver[1], g.ver[2]);
          const V3 P = add(add(llc, scale(hor, u)), scale(ver, v));
          if (g.kind == ZRT_LENS_ORTHO) {
            o = P;
            tgt = add(o, aw);
          } else {  // pinhole; the thin lens: an origin on the lens, the plane is the focal plane
            o = g.kind == ZRT_LENS_THIN ? add(add(org, scale(au, la)), scale(av, lb)) : org;
            tgt = P;
          }
        }
        d = unit(sub(tgt, o));
        depth_left = a.max_depth;
        in_sample = true;
      }
      // ---- one rayColor step (raytrace.zig:62-100)
      bool path_end = false, sky = false;
      V3 L = mk(0.0f, 0.0f, 0.0f);
      if (depth_left == 0) {
        ++c_depth;
        path_end = true;
      } else {
        float best_t;
        int best;
        closest_hit<MODE, StackT>(a, o, d, stk, lds_top, gl, best_t, best);
        shade_step<false, Rng<PRNG>>(a, mats, ar, rng, best, best_t, o, d, depth_left, path_end, sky, L, c_bg, c_refl,
                                     c_shade, c_tex, coh);
      }
      if (path_end) {
        const V3 col = sky ? att_product<false>(a, mats, ar, a.max_depth - depth_left, L, coh) : L;
        acc_r += col.x;
        acc_g += col.y;
        acc_b += col.z;
        // (shade_step pushes a scatter's row while depth_left > 1: the one at depth 1 is never read)
        deepest = max(deepest, a.max_depth - depth_left - (depth_left == 0 && a.max_depth != 0 ? 1u : 0u));
        in_sample = false;
        if (++sample == s_end) break;  // the chunk's sequential sum is complete
      }
    }
    a.partial[cj * g.n + slot0 + lane] = make_float4(acc_r, acc_g, acc_b, 0.0f);
  }
  wave_add_u64(&a.counters[kDepthHits], c_depth);
  wave_add_u64(&a.counters[kReflections], c_refl);
  wave_add_u64(&a.counters[kBackground], c_bg);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) deepest = max(deepest, (uint32_t)__shfl_xor((int)deepest, off));
  if (lane == 0 && deepest) atomicMax(&a.counters[kRqDeepestSlot], (unsigned long long)deepest);
}

// Behind camera_kernel, one lane per slot: radiance_finish_kernel with the slot mapped to
// its pixel.  sum and rgb are whole-frame buffers indexed by R = y * width + x; a slot
// outside the rectangle reads and writes nothing, so the frame's other pixels stay.
// moments (zrt_ctx_camera_moments; block-uniform): sum[R].w is Q, accumulate_kernel's second
// moment - per parked sum S_j of the round's first q_chunks (all but a ragged last one), l =
// (S_j.r + S_j.g) + S_j.b, Q = Q + l * l, in chunk order, from 0 where zero_first, else from
// sum[R].w; NaN after a device error.  Without it .w is written 0, as before.
__global__ void camera_finish_kernel(const float4* __restrict__ partial, const CameraArgs g, uint32_t n_chunks,
                                     uint32_t zero_first, float4* __restrict__ sum, float* __restrict__ rgb,
                                     float scale, uint32_t final, const unsigned long long* __restrict__ error_flag,
                                     uint32_t moments, uint32_t q_chunks) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= g.n) return;
  const uint32_t tile = i >> 6, l = i & 63u;
  const uint32_t ty = tile / g.tiles_w, tx = tile - ty * g.tiles_w;
  const uint32_t lx = tx * 8u + (l & 7u), ly = ty * 8u + (l >> 3);
  if (lx >= g.w || ly >= g.h) return;
  const uint64_t R = (uint64_t)(g.y0 + ly) * g.width + (g.x0 + lx);
  float4 s = zero_first ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : sum[R];
  float q = moments ? s.w : 0.0f;
  for (uint32_t j = 0; j < n_chunks; ++j) {
    const float4 p = partial[(uint64_t)j * g.n + i];
    s.x += p.x;
    s.y += p.y;
    s.z += p.z;
    if (moments && j < q_chunks) {  // (a ragged last chunk is left out of the second moment)
      const float lum = (p.x + p.y) + p.z;
      q = q + lum * lum;
    }
  }
  if (final && *error_flag != 0ull) {
    s.x = s.y = s.z = __builtin_nanf("");
    if (moments) q = __builtin_nanf("");
  }
  sum[R] = make_float4(s.x, s.y, s.z, q);
  if (final && rgb) {
    rgb[3ull * R + 0] = s.x * scale;
    rgb[3ull * R + 1] = s.y * scale;
    rgb[3ull * R + 2] = s.z * scale;
  }
}

// ---------------------------------------------------------------------------
// host side (kernels.hpp): what must see a kernel symbol or a device template
// ---------------------------------------------------------------------------
namespace {
template <int MODE, int PRNG, bool STATS, class StackT, bool LEAN = false, bool ONE_SPHERE = false>
void* kernel_ptr() {
  return reinterpret_cast<void*>(&render_kernel<MODE, PRNG, STATS, StackT, LEAN, ONE_SPHERE>);
}

template <int PRNG, bool STATS>
void* select_kernel_ps(int mode, bool stk16) {
  if (mode == 0) return kernel_ptr<0, PRNG, STATS, uint16_t>();  // list mode: no stack
  if (mode == 6) return kernel_ptr<6, PRNG, STATS, uint16_t>();  // list mode, per-lane work items
  if (mode == 1) return stk16 ? kernel_ptr<1, PRNG, STATS, uint16_t>() : kernel_ptr<1, PRNG, STATS, uint32_t>();
  if (mode == 3) return stk16 ? kernel_ptr<3, PRNG, STATS, uint16_t>() : kernel_ptr<3, PRNG, STATS, uint32_t>();
  if (mode == 4) return stk16 ? kernel_ptr<4, PRNG, STATS, uint16_t>() : kernel_ptr<4, PRNG, STATS, uint32_t>();
  if (mode == 5) return stk16 ? kernel_ptr<5, PRNG, STATS, uint16_t>() : kernel_ptr<5, PRNG, STATS, uint32_t>();
  if (mode == 7) return stk16 ? kernel_ptr<7, PRNG, STATS, uint16_t>() : kernel_ptr<7, PRNG, STATS, uint32_t>();
  if (mode == 8) return stk16 ? kernel_ptr<8, PRNG, STATS, uint16_t>() : kernel_ptr<8, PRNG, STATS, uint32_t>();
  if (mode == 9) return stk16 ? kernel_ptr<9, PRNG, STATS, uint16_t>() : kernel_ptr<9, PRNG, STATS, uint32_t>();
  return stk16 ? kernel_ptr<2, PRNG, STATS, uint16_t>() : kernel_ptr<2, PRNG, STATS, uint32_t>();
}
}  // namespace
#ifdef ZRT_ISA_KERNEL
// tools/isa.sh: device assembly of ONE render kernel (register / spill probes in
// seconds instead of minutes); ZRT_ISA_KERNEL = MODE, PRNG, STATS, StackT[, true: the lean kernel[, true: its
// one-sphere sibling]]
void* select_kernel(int, uint32_t, bool, bool, bool) { return kernel_ptr<ZRT_ISA_KERNEL>(); }
#else
// lean: the lean kernel of the timed lockstep FAST loop (plan_launch decides; four kernels)
void* select_kernel(int mode, uint32_t prng, bool stats, bool stk16, bool lean) {
  if (lean) {
    if (mode != 3 || stats) throw Error(ZRT_E_UNSUPPORTED, "no lean kernel for this loop");
    if (prng == ZRT_PRNG_XOSHIRO256)
      return stk16 ? kernel_ptr<3, ZRT_PRNG_XOSHIRO256, false, uint16_t, true>()
                   : kernel_ptr<3, ZRT_PRNG_XOSHIRO256, false, uint32_t, true>();
    return stk16 ? kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, false, uint16_t, true>()
                 : kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, false, uint32_t, true>();
  }
  if (prng == ZRT_PRNG_XOSHIRO256)
    return stats ? select_kernel_ps<ZRT_PRNG_XOSHIRO256, true>(mode, stk16)
                 : select_kernel_ps<ZRT_PRNG_XOSHIRO256, false>(mode, stk16);
  return stats ? select_kernel_ps<ZRT_PRNG_XOROSHIRO128, true>(mode, stk16)
               : select_kernel_ps<ZRT_PRNG_XOROSHIRO128, false>(mode, stk16);
}
#endif

// every other kernel-pointer table is empty under ZRT_ISA_KERNEL (tools/isa.sh: one render kernel alone).
// The templates are instantiated, and their kernels laid out in the code object, in the order
// of the functions from here on (probe, sort, features, trace, debug_rng): moving one reorders the
// device assembly, which is otherwise compared byte for byte across host-only changes.
#ifdef ZRT_ISA_KERNEL
#define ZRT_STK(K, ...) ((void)stk16, static_cast<void*>(nullptr))
#else
#define ZRT_STK(K, ...) (stk16 ? reinterpret_cast<void*>(&K<__VA_ARGS__, uint16_t>) \
                               : reinterpret_cast<void*>(&K<__VA_ARGS__, uint32_t>))
#endif
void* probe_kernel(uint32_t prng, bool stk16) {
  return prng == ZRT_PRNG_XOSHIRO256 ? ZRT_STK(schedule_probe_kernel, ZRT_PRNG_XOSHIRO256)
                                     : ZRT_STK(schedule_probe_kernel, ZRT_PRNG_XOROSHIRO128);
}
void* sky_kernel_ptr(uint32_t prng, bool stats) {
#ifdef ZRT_ISA_KERNEL
  return nullptr;
#else
  if (prng == ZRT_PRNG_XOSHIRO256)
    return stats ? reinterpret_cast<void*>(&sky_kernel<ZRT_PRNG_XOSHIRO256, true>)
                 : reinterpret_cast<void*>(&sky_kernel<ZRT_PRNG_XOSHIRO256, false>);
  return stats ? reinterpret_cast<void*>(&sky_kernel<ZRT_PRNG_XOROSHIRO128, true>)
               : reinterpret_cast<void*>(&sky_kernel<ZRT_PRNG_XOROSHIRO128, false>);
#endif
}
// the one-sphere kernels: the lean timed flavour and the (general) STATS flavour, both
// generators, both stack widths - eight
void* one_sphere_kernel(uint32_t prng, bool stats, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  return nullptr;
#else
  if (prng == ZRT_PRNG_XOSHIRO256) {
    if (stats)
      return stk16 ? kernel_ptr<3, ZRT_PRNG_XOSHIRO256, true, uint16_t, false, true>()
                   : kernel_ptr<3, ZRT_PRNG_XOSHIRO256, true, uint32_t, false, true>();
    return stk16 ? kernel_ptr<3, ZRT_PRNG_XOSHIRO256, false, uint16_t, true, true>()
                 : kernel_ptr<3, ZRT_PRNG_XOSHIRO256, false, uint32_t, true, true>();
  }
  if (stats)
    return stk16 ? kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, true, uint16_t, false, true>()
                 : kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, true, uint32_t, false, true>();
  return stk16 ? kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, false, uint16_t, true, true>()
               : kernel_ptr<3, ZRT_PRNG_XOROSHIRO128, false, uint32_t, true, true>();
#endif
}
hipError_t sort_tiles(void* temp, size_t* temp_bytes, const uint32_t* cost, uint32_t* cost_sorted, const uint32_t* ids,
                      uint32_t* order, uint32_t n, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairsDescending(temp, *temp_bytes, cost, cost_sorted, ids, order, int(n), 0, 32, st);
}
void* features_kernel_ptr(int mode, bool stk16) {
  return mode == 0 ? ZRT_STK(features_kernel, 0) : mode == 1 ? ZRT_STK(features_kernel, 1)
       : mode == 2 ? ZRT_STK(features_kernel, 2) : mode == 8 ? ZRT_STK(features_kernel, 8) : ZRT_STK(features_kernel, 3);
}
void* trace_kernel_ptr(int mode, bool stk16) {
  return mode == 0 ? ZRT_STK(trace_kernel, 0) : mode == 1 ? ZRT_STK(trace_kernel, 1)
       : mode == 2 ? ZRT_STK(trace_kernel, 2) : mode == 8 ? ZRT_STK(trace_kernel, 8) : ZRT_STK(trace_kernel, 3);
}
#undef ZRT_STK

// One launch function per small kernel (kernels.hpp)
namespace {
template <class... P, class... A>
hipError_t launch(void (*kernel)(P...), uint32_t grid, uint32_t block, hipStream_t st, A... args) {
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, args...);
  return hipGetLastError();
}
}  // namespace
hipError_t launch_finalize(hipStream_t st, const float4* partial, float* out, uint32_t n_slots, uint32_t n_chunks,
                           uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound, uint32_t height,
                           float color_scale, const unsigned long long* error_flag) {
  return launch(finalize_kernel, (n_slots + 255) / 256, 256, st, partial, out, n_slots, n_chunks, world, rank,
                    tiles_x, xbound, height, color_scale, error_flag);
}
hipError_t launch_accumulate(hipStream_t st, const float4* partial, float4* accum, float* out, uint32_t n_slots,
                             uint32_t pass_chunks, uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound,
                             uint32_t height, float prev_scale, float new_scale, uint32_t q_chunks,
                             const unsigned long long* error_flag, unsigned long long* metrics) {
  return launch(accumulate_kernel, (n_slots + 255) / 256, 256, st, partial, accum, out, n_slots, pass_chunks, world,
                    rank, tiles_x, xbound, height, prev_scale, new_scale, q_chunks, error_flag, metrics);
}
hipError_t launch_resolve(hipStream_t st, const float4* partial, float4* accum, float* out, const uint32_t* active,
                          uint32_t n_active, uint32_t my_tiles, uint32_t pass_chunks, uint32_t world, uint32_t rank,
                          uint32_t tiles_x, uint32_t xbound, uint32_t height, float prev_scale, float new_scale,
                          uint32_t q_chunks, float tolerance, uint32_t decide, uint32_t level_samples,
                          uint32_t* tile_done, const unsigned long long* error_flag, unsigned long long* metrics) {
  return launch(resolve_kernel, (n_active + 3) / 4, 256, st, partial, accum, out, active, n_active, my_tiles,
                    pass_chunks, world, rank, tiles_x, xbound, height, prev_scale, new_scale, q_chunks, tolerance,
                    decide, level_samples, tile_done, error_flag, metrics);
}
hipError_t launch_compact(hipStream_t st, const uint32_t* in, uint32_t n, const uint32_t* tile_done, uint32_t* out,
                          uint32_t* count) {
  return launch(compact_kernel, 1, kCompactBlock, st, in, n, tile_done, out, count);
}
hipError_t launch_compact_class(hipStream_t st, const uint32_t* in, uint32_t n, const uint32_t* cls, uint32_t word,
                                uint32_t* out, uint32_t* count) {
  return launch(compact_class_kernel, 1, kCompactBlock, st, in, n, cls, word, out, count);
}
hipError_t launch_assemble(hipStream_t st, const float* gathered, float* frame, const uint32_t* rank_base,
                           uint32_t world, uint32_t tiles_x, uint32_t xbound, uint32_t height, uint32_t width,
                           uint32_t total, uint32_t stride_px, uint32_t n_tiles) {
  return launch(assemble_kernel<3>, (total + 255) / 256, 256, st, gathered, frame, rank_base, world, tiles_x, xbound,
                    height, width, total, stride_px, n_tiles);
}
hipError_t launch_variance(hipStream_t st, const float4* accum, const float2* tile_plan, float* out, uint32_t n_slots,
                           uint32_t world, uint32_t rank, uint32_t tiles_x, uint32_t xbound, uint32_t height,
                           const unsigned long long* error_flag) {
  return launch(variance_kernel, (n_slots + 255) / 256, 256, st, accum, tile_plan, out, n_slots, world, rank, tiles_x,
                    xbound, height, error_flag);
}
hipError_t launch_assemble_plane(hipStream_t st, const float* gathered, float* frame, const uint32_t* rank_base,
                                 uint32_t world, uint32_t tiles_x, uint32_t xbound, uint32_t height, uint32_t width,
                                 uint32_t total, uint32_t stride_px, uint32_t n_tiles) {
  return launch(assemble_kernel<1>, (total + 255) / 256, 256, st, gathered, frame, rank_base, world, tiles_x, xbound,
                    height, width, total, stride_px, n_tiles);
}
hipError_t launch_features_error(hipStream_t st, float4* out, uint64_t n_f4, const unsigned long long* error_flag) {
  const uint32_t grid = uint32_t(n_f4 + 255 < 4096ull * 256 ? (n_f4 + 255) / 256 : 4096);
  return launch(features_error_kernel, grid, 256, st, out, n_f4, error_flag);
}
hipError_t launch_debug_math(int fn, const float* x, const float* y, float* out, uint32_t n) {
  return launch(debug_math_kernel, (n + 255) / 256, 256, 0, fn, x, y, out, n);
}
hipError_t launch_debug_division(uint64_t n, unsigned long long* counts) {
  return launch(debug_division_kernel, 8192, 256, 0, n, counts);
}
hipError_t launch_debug_rng(uint32_t prng, uint64_t key, unsigned long long* out, uint32_t n) {
  if (prng == ZRT_PRNG_XOSHIRO256) return launch(debug_rng_kernel<ZRT_PRNG_XOSHIRO256>, 1, 64, 0, key, out, n);
  return launch(debug_rng_kernel<ZRT_PRNG_XOROSHIRO128>, 1, 64, 0, key, out, n);
}
// The ray queries' kernels (queries.cpp), after every older one: they add to the end of the
// code object.  anyhit_kernel by traversal mode; FAST (3) reads the full wide nodes only.
void* anyhit_kernel_ptr(int mode, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  (void)mode; (void)stk16;
  return nullptr;
#else
#define ZRT_ANYHIT(M) (stk16 ? reinterpret_cast<void*>(&anyhit_kernel<M, uint16_t>) \
                             : reinterpret_cast<void*>(&anyhit_kernel<M, uint32_t>))
  return mode == 0 ? ZRT_ANYHIT(0) : mode == 1 ? ZRT_ANYHIT(1) : mode == 2 ? ZRT_ANYHIT(2) : ZRT_ANYHIT(3);
#undef ZRT_ANYHIT
#endif
}
hipError_t launch_trace_finish(hipStream_t st, float* t, int32_t* prim, uint32_t n, const uint32_t* slot_prim,
                               const unsigned long long* error_flag) {
  return launch(trace_finish_kernel, (n + 255) / 256, 256, st, t, prim, n, slot_prim, error_flag);
}
hipError_t launch_anyhit_error(hipStream_t st, uint8_t* out, uint32_t n, const unsigned long long* error_flag) {
  return launch(anyhit_error_kernel, (n + 255) / 256, 256, st, out, n, error_flag);
}
// Ambient occlusion (ao.cpp), after the queries': ao_kernel by traversal mode (as anyhit_kernel), PRNG and
// stack width.
void* ao_kernel_ptr(int mode, uint32_t prng, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  (void)mode; (void)prng; (void)stk16;
  return nullptr;
#else
#define ZRT_AO_S(M, R) (stk16 ? reinterpret_cast<void*>(&ao_kernel<M, R, uint16_t>) \
                              : reinterpret_cast<void*>(&ao_kernel<M, R, uint32_t>))
#define ZRT_AO(M) (prng == ZRT_PRNG_XOSHIRO256 ? ZRT_AO_S(M, ZRT_PRNG_XOSHIRO256) : ZRT_AO_S(M, ZRT_PRNG_XOROSHIRO128))
  return mode == 0 ? ZRT_AO(0) : mode == 1 ? ZRT_AO(1) : mode == 2 ? ZRT_AO(2) : ZRT_AO(3);
#undef ZRT_AO
#undef ZRT_AO_S
#endif
}
hipError_t launch_ao_finish(hipStream_t st, const AoArgs& g, uint32_t width, uint32_t height, uint32_t xbound,
                            const float4* feat, uint32_t* clear, float* ao, const uint32_t* plane,
                            const unsigned long long* error_flag) {
  const uint64_t n_px = uint64_t(width) * height;
  const uint32_t grid = uint32_t(n_px + 255 < 4096ull * 256 ? (n_px + 255) / 256 : 4096);
  return launch(ao_finish_kernel, grid, 256, st, g, width, height, xbound, feat, clear, ao, plane, error_flag);
}
// Radiance queries (radiance.cpp), after AO's: radiance_kernel by traversal mode (as anyhit_kernel), PRNG and
// stack width.
void* radiance_kernel_ptr(int mode, uint32_t prng, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  (void)mode; (void)prng; (void)stk16;
  return nullptr;
#else
#define ZRT_RQ_S(M, R) (stk16 ? reinterpret_cast<void*>(&radiance_kernel<M, R, uint16_t>) \
                              : reinterpret_cast<void*>(&radiance_kernel<M, R, uint32_t>))
#define ZRT_RQ(M) (prng == ZRT_PRNG_XOSHIRO256 ? ZRT_RQ_S(M, ZRT_PRNG_XOSHIRO256) : ZRT_RQ_S(M, ZRT_PRNG_XOROSHIRO128))
  return mode == 0 ? ZRT_RQ(0) : mode == 1 ? ZRT_RQ(1) : mode == 2 ? ZRT_RQ(2) : ZRT_RQ(3);
#undef ZRT_RQ
#undef ZRT_RQ_S
#endif
}
hipError_t launch_radiance_finish(hipStream_t st, const float4* partial, uint32_t n, uint32_t n_chunks,
                                  uint32_t zero_first, float4* sum, float* rgb, float scale, uint32_t final,
                                  const unsigned long long* error_flag) {
  return launch(radiance_finish_kernel, uint32_t((uint64_t(n) + 255) / 256), 256, st, partial, n, n_chunks, zero_first,
                sum, rgb, scale, final, error_flag);
}
// Camera queries (camera_query.cpp): camera_kernel by radiance_kernel's modes, PRNG and stack width.
void* camera_kernel_ptr(int mode, uint32_t prng, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  (void)mode; (void)prng; (void)stk16;
  return nullptr;
#else
#define ZRT_CQ_S(M, R) (stk16 ? reinterpret_cast<void*>(&camera_kernel<M, R, uint16_t>) \
                              : reinterpret_cast<void*>(&camera_kernel<M, R, uint32_t>))
#define ZRT_CQ(M) (prng == ZRT_PRNG_XOSHIRO256 ? ZRT_CQ_S(M, ZRT_PRNG_XOSHIRO256) : ZRT_CQ_S(M, ZRT_PRNG_XOROSHIRO128))
  return mode == 0 ? ZRT_CQ(0) : mode == 1 ? ZRT_CQ(1) : mode == 2 ? ZRT_CQ(2) : ZRT_CQ(3);
#undef ZRT_CQ
#undef ZRT_CQ_S
#endif
}
hipError_t launch_camera_finish(hipStream_t st, const float4* partial, const CameraArgs& g, uint32_t n_chunks,
                                uint32_t zero_first, float4* sum, float* rgb, float scale, uint32_t final,
                                const unsigned long long* error_flag, uint32_t moments, uint32_t q_chunks) {
  return launch(camera_finish_kernel, uint32_t((uint64_t(g.n) + 255) / 256), 256, st, partial, g, n_chunks, zero_first,
                sum, rgb, scale, final, error_flag, moments, q_chunks);
}
// Lens features (camera_query.cpp), after the camera query's: lens_features_kernel by anyhit_kernel's modes.
void* lens_features_kernel_ptr(int mode, bool stk16) {
#ifdef ZRT_ISA_KERNEL
  (void)mode; (void)stk16;
  return nullptr;
#else
#define ZRT_LF(M) (stk16 ? reinterpret_cast<void*>(&lens_features_kernel<M, uint16_t>) \
                         : reinterpret_cast<void*>(&lens_features_kernel<M, uint32_t>))
  return mode == 0 ? ZRT_LF(0) : mode == 1 ? ZRT_LF(1) : mode == 2 ? ZRT_LF(2) : ZRT_LF(3);
#undef ZRT_LF
#endif
}
hipError_t launch_lens_features_error(hipStream_t st, float4* out, const CameraArgs& g,
                                      const unsigned long long* error_flag) {
  return launch(lens_features_error_kernel, uint32_t((uint64_t(g.n) + 255) / 256), 256, st, out, g, error_flag);
}

const KernelConfig& kernel_config() {
  static const KernelConfig k = {
      ZRT_WAVES_WIDE, ZRT_WAVES_WF, ZRT_WAVES_POOL, ZRT_WAVES_LIST, ZRT_WAVES_PER_SIMD,
      ZRT_ATT_ROWS_LOCK, ZRT_ATT_ROWS_WF, ZRT_ATT_ROWS_POOL, ZRT_ATT_ROWS_LIST,
      ZRT_STACK_ROWS_LOCK, ZRT_SYNC_SAMPLES, ZRT_PROBE_SPP,
      kOctCopies,
      {LaneState<ZRT_PRNG_XOROSHIRO128>::kWords, LaneState<ZRT_PRNG_XOSHIRO256>::kWords},
      kBlockPaths,
      kKernelLayout,
      kPaxisM,
      ZRT_PROFILE != 0,
  };
  return k;
}
}  // namespace zrt
