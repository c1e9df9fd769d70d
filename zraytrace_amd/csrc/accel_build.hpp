// accel_build.hpp — wide SAH tree over the reference BVH's leaves (see accel_build.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace zrt {

struct float4v {  // host-side float4 (same layout as HIP's float4)
  float v[4];
};

// One reference leaf (bvh.zig:132-143): its exact box and its one or two
// primitives as render.hip primitive-slot refs (-(2*slot + kind) - 1).
struct RefLeaf {
  float mn[3], mx[3];
  int32_t prim_a, prim_b;
};

// The wide tree's encoding (WideBvh::layout), recorded by build_wide_bvh and
// compared with what the selected kernel decodes before any launch, on the host
// and again by the kernel itself (render.hip kKernelLayout): a kernel variant that
// did not decode biased sphere refs used them as primitive indices and faulted
// (VERDICT r03 #3).  A mismatch is ZRT_E_UNSUPPORTED, never a launch.
constexpr uint32_t kLayoutVersion = 1u << 8;      // 128-B nodes, inline leaves, refs as below
constexpr uint32_t kLayoutSphereSlots = 1u << 0;  // sphere leaf refs stored - kSphereSlotBias ...
constexpr uint32_t kLayoutSphereFirst = 1u << 1;  // ... in a node's first slots

struct WideBvh {
  std::vector<float4v> nodes;   // 8 per wide node, node 0 = root
  uint32_t n_nodes = 0, n_leaves = 0, depth = 0, max_stack = 0;
  uint32_t n_top = 0;           // nodes of the top levels, stored first (0 .. n_top-1)
  std::vector<uint32_t> level_end;  // nodes of the first 1, 2, .. top levels (breadth-first prefix)
  uint32_t layout = 0;          // kLayout* bits of this encoding
};

// A leaf slot holding a sphere stores its ref a minus kSphereSlotBias (below
// -2^30, where no other ref lies): render.hip opens such slots with the
// reference's loose test against t_max = +inf (DESIGN.md §3 "Spheres") and adds
// the bias back before testing the primitives.
constexpr int32_t kSphereSlotBias = int32_t(1) << 30;

// top_levels: how many levels (root = 1) are stored first, breadth-first.
// inflate: inner children's boxes are stored grown on every side by this much
// times their own largest |coordinate| (rounded outward); leaf children keep
// the reference leaf's box bit for bit.
// sphere_grow: inner children whose subtree holds a sphere are grown by this
// much more (absolute): the rounded sphere test's reach beyond the sphere.
// mark_spheres: leaf slots holding a sphere carry ref a - kSphereSlotBias (as
// render.hip's kernels decode them: kKernelLayout).
WideBvh build_wide_bvh(const std::vector<RefLeaf>& leaves, uint32_t top_levels = 2, float inflate = 0.0f,
                       float sphere_grow = 0.0f, bool mark_spheres = false);

// primitive-slot ref of render.hip, -(2*slot + kind) - 1: kind 0 is a sphere
inline bool ref_is_sphere(int32_t ref) { return ref < 0 && ((-(int64_t(ref) + 1)) & 1) == 0; }

}  // namespace zrt

namespace zrt {

// Compressed wide nodes for trees past the caches (render.hip wide_iter_q,
// DESIGN.md §3 "Compressed nodes"): 64 B per node instead of 128 B.
//   node = 4 x float4 (16 words), per ray-octant copy:
//     w0-2  origin.xyz (f32), w3 the per-axis step exponents, biased by 127
//           (step_k = 2^(e_k - 127), a normal float; bits 0-7 x, 8-15 y, 16-23 z)
//     w4-6  near planes x, y, z of slots 0..3 as bytes (byte k = slot k)
//     w7-9  far planes x, y, z (bytes); near / far pre-swapped per octant as
//           the full nodes' planes are
//     w10-13 refs of slots 0..3: inner child = node index (>= 0); leaf =
//           -(leaf record + 1), minus kSphereSlotBias for a sphere leaf;
//           empty slot = kEmptyRef
//     w14-15 0
//   A plane is origin + q * step, computed exactly in f32 (origin is a multiple
//   of step and |origin / step| + 255 < 2^24), and quantized outward: every
//   child box contains the full node's box of that slot, so the culls stay
//   supersets (any containing box is allowed, accel_build.cpp's header).
//   leaf record = 2 x float4: {min.xyz, prim ref a}, {max.xyz, prim ref b}: the
//   reference leaf's own box bit for bit (the loose test and the hazard entry
//   read it) and its one or two primitive-slot refs.
constexpr int32_t kEmptyRef = INT32_MIN;
constexpr uint32_t kQuantNodeF4 = 4, kLeafRecF4 = 2;

struct QuantWide {
  std::vector<float4v> nodes;   // 8 octant copies, copy-major: copy o at o * n_nodes * 4
  std::vector<float4v> leaves;  // kLeafRecF4 per leaf record
  uint32_t n_nodes = 0, n_leaves = 0;
  bool ok = false;  // false: a box could not be quantized (a non-finite plane): use the full nodes
};

// The 8 octant copies of `w`'s nodes (full format, unswapped planes) compressed.
QuantWide quantize_wide(const WideBvh& w);

}  // namespace zrt
