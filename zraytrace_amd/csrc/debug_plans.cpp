// debug_plans.cpp - the zrt_debug_* entry points that need no device: they report
// or check what the planner and the flattener decide (planner.cpp, flatten.cpp) and
// make no HIP runtime call, so a host sanitizer build links and drives them
// (tools/sanitize).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "accel_build.hpp"
#include "host.hpp"

using zrt::fail;

int zrt_debug_pass_plan(const zrt_params* params, uint32_t done, uint32_t n_samples, zrt_pass_plan* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  return zrt::plan_pass(params, done, n_samples, out);
}

int zrt_debug_adapt_plan(const zrt_params* params, const zrt_adaptive* adaptive, uint32_t* levels, uint32_t cap,
                         uint32_t* n_levels) {
  if (!n_levels || (cap && !levels)) return fail(ZRT_E_INVALID, "null argument");
  std::vector<uint32_t> L;
  const int rc = zrt::plan_adapt(params, adaptive, &L);
  if (rc) return rc;
  *n_levels = uint32_t(L.size());
  for (uint32_t k = 0; k < cap && k < L.size(); ++k) levels[k] = L[k];
  return ZRT_OK;
}

int zrt_debug_variance_plan(const zrt_params* params, uint32_t n_samples, zrt_variance_plan* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  return zrt::plan_variance(params, n_samples, out);
}

int zrt_debug_reproject_plan(const zrt_camera* prev, const zrt_params* params, zrt_reproject_plan* out) {
  if (!out) return fail(ZRT_E_INVALID, "null argument");
  return zrt::plan_reproject(prev, params, out);
}

int zrt_debug_camera_plan(const zrt_params* params, const zrt_camera_query* query, uint32_t cu_count,
                          uint64_t partial_cap_bytes, zrt_camera_plan* out) {
  return zrt::plan_camera(params, query, cu_count, partial_cap_bytes, out);
}

int zrt_debug_octant_offsets(uint32_t stride_f4, uint32_t n_top, uint32_t node_f4) {
  try {
    zrt::check_octant_offsets(stride_f4, n_top, node_f4);
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_lds_plans(const zrt_scene* scene, uint32_t* n_checked) {
  if (!n_checked) return fail(ZRT_E_INVALID, "null argument");
  *n_checked = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  try {
    zrt::HostScene h;
    // (the host BVH build: no device; the compressed nodes built too, so their
    // plans are checked with the top levels they really keep in LDS)
    zrt::flatten_scene(&h, scene, scene->n_prims > 10, -1, scene->n_prims > 10 ? 1 : 0);
    const uint32_t n_mats = uint32_t(h.mats.size());
    const uint32_t ref_depth = h.use_bvh ? h.bvh_depth + 2 : 0;
    std::string where;
    for (int mode : {0, 1, 2, 3}) {
      for (int loop = 0; loop < (mode == 3 ? 3 : 1); ++loop) {  // lockstep, wavefront, path pool
        for (bool stk16 : {true, false}) {
          for (uint32_t prng : {uint32_t(ZRT_PRNG_XOROSHIRO128), uint32_t(ZRT_PRNG_XOSHIRO256)}) {
            for (uint32_t depth : {0u, 1u, 2u, 5u, 20u, 50u}) {
              for (uint32_t nf4 : {8u, 4u}) {  // full / compressed wide nodes (the path pool only)
                if (nf4 == 4u && (loop != 2 || !h.q_ok)) continue;
                // the plan as the environment has it, and (FAST, 16-bit stack) with the LDS
                // rows capped as ZRT_STACK_LDS_ROWS16 caps them
                for (uint32_t cap : {zrt::stack_rows_cap(), 1u, 2u, 4u}) {
                  const bool capped = cap != zrt::stack_rows_cap();
                  if (capped && !(mode == 3 && stk16)) continue;
                  const uint32_t sd = mode == 3 ? std::max(h.wide_stack, ref_depth) : ref_depth;
                  where = "mode " + std::to_string(mode) + " loop " + std::to_string(loop) + " stk16 " +
                          std::to_string(int(stk16)) + " prng " + std::to_string(prng) + " depth " +
                          std::to_string(depth) + " node_f4 " + std::to_string(nf4) +
                          (capped ? " stack rows capped at " + std::to_string(cap) : std::string());
                  try {
                    (void)zrt::plan_lds(nf4 == 4u ? h.q_top : h.n_top, n_mats, mode, stk16, sd, depth, loop == 1,
                                        loop == 2, prng, nf4, cap);
                  } catch (const zrt::Error& e) {
                    throw zrt::Error(e.code, std::string(e.what()) + " (" + where + ")");
                  }
                  ++*n_checked;
                }
              }
            }
          }
        }
      }
    }
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_buffer_plans(const zrt_scene* scene, uint32_t legacy, uint32_t* n_checked) {
  if (!n_checked) return fail(ZRT_E_INVALID, "null argument");
  *n_checked = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (scene->n_prims <= 10) return ZRT_OK;  // no tree: no FAST launch, no probe
  try {
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, true, -1, 1);
    const uint32_t n_mats = uint32_t(h.mats.size());
    const uint32_t sd = std::max(h.wide_stack, h.bvh_depth + 2);  // zrt_render's FAST stack depth
    for (int loop = 0; loop < 3; ++loop) {  // the render launch: lockstep, wavefront, path pool
      for (bool stk16 : {true, false}) {
        for (uint32_t prng : {uint32_t(ZRT_PRNG_XOROSHIRO128), uint32_t(ZRT_PRNG_XOSHIRO256)}) {
          for (uint32_t depth : {0u, 1u, 2u, 4u, 5u, 6u, 13u, 20u, 50u}) {
            for (uint32_t nf4 : {8u, 4u}) {
              if (nf4 == 4u && (loop != 2 || !h.q_ok)) continue;
              for (uint32_t grid : {64u, 1536u, 2048u}) {  // blocks (the probe: at most the render's)
               // the plans as the environment has them, and (16-bit stack) with the LDS rows
               // capped as ZRT_STACK_LDS_ROWS16 caps them: more overflow rows for both launches
               for (uint32_t cap : {zrt::stack_rows_cap(), 1u, 2u, 4u}) {
                const bool capped = cap != zrt::stack_rows_cap();
                if (capped && !stk16) continue;
                const std::string where = "loop " + std::to_string(loop) + " stk16 " + std::to_string(int(stk16)) +
                                          " prng " + std::to_string(prng) + " depth " + std::to_string(depth) +
                                          " node_f4 " + std::to_string(nf4) + " grid " + std::to_string(grid) +
                                          (capped ? " stack rows capped at " + std::to_string(cap) : std::string());
                // zrt_render's sizing: the render launch's need, then (schedule_tiles) the
                // probe's, the buffers grown to the larger of the two
                const zrt::LdsPlan lp = zrt::plan_lds(nf4 == 4u ? h.q_top : h.n_top, n_mats, 3, stk16, sd, depth,
                                                      loop == 1, loop == 2, prng, nf4, cap);
                const uint64_t n_lanes = uint64_t(grid) * zrt::kBlock;
                const uint64_t n_paths = loop == 2 ? uint64_t(grid) * zrt::kernel_config().block_paths : n_lanes;
                const zrt::BufNeed rn = zrt::buffer_need(lp, depth, sd, n_paths, n_lanes, stk16);
                const zrt::LdsPlan pp = zrt::plan_lds(h.n_top, n_mats, 3, stk16, sd, depth, false, false, prng, 8, cap);
                const zrt::BufNeed pn = zrt::buffer_need(pp, depth, sd, n_lanes, n_lanes, stk16);
                uint64_t att = rn.att_elems, ovf = std::max(rn.ovf_bytes, pn.ovf_bytes);
                // legacy = 1: the sizing before commit 4072f5f, where the probe shared the
                // render launch's attenuation rows without growing them
                if (!legacy) att = std::max(att, pn.att_elems);
                try {
                  zrt::check_buffers("scheduling probe", pn, att, ovf);
                  zrt::check_buffers("render launch", rn, att, ovf);
                } catch (const zrt::Error& e) {
                  throw zrt::Error(e.code, std::string(e.what()) + " (" + where + ")");
                }
                ++*n_checked;
               }
              }
            }
          }
        }
      }
    }
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_launch_plan(const zrt_scene* scene, const zrt_params* params, zrt_launch_plan* out) {
  if (!params || !out) return fail(ZRT_E_INVALID, "null argument");
  std::memset(out, 0, sizeof(*out));
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (params->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;  // (zrt_ctx_create)
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, use_bvh, -1);
    const zrt::LaunchPlan P = zrt::plan_launch(zrt::shape_of(h), params);
    out->mode = uint32_t(P.mode);
    out->kmode = uint32_t(P.kmode);
    out->sampling_loop = zrt::reported_loop(P.kmode);
    out->stk16 = P.stk16;
    out->wf = P.wf;
    out->pool = P.pool;
    out->qnodes = P.qn;
    out->guard_on = P.guard_on;
    out->stack_depth = P.stack_depth;
    out->stack_rows = P.lp.stack_rows;
    out->att_rows = P.lp.att_rows;
    out->att_rows_per_path = zrt::att_rows_per_path(P.lp, params->max_depth);
    out->mats_in_lds = P.lp.mats_in_lds;
    out->lds_bytes = uint32_t(P.lp.bytes);
    out->ovf_bytes_per_lane = zrt::buffer_need(P.lp, params->max_depth, P.stack_depth, 1, 1, P.stk16).ovf_bytes;
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_lean_kernel(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params, uint32_t* lean) {
  if (!camera || !params || !lean) return fail(ZRT_E_INVALID, "null argument");
  *lean = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (params->traversal > ZRT_TRAVERSAL_BINARY) return fail(ZRT_E_INVALID, "unknown traversal");
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;  // (zrt_ctx_create)
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, use_bvh, -1);
    const zrt::LaunchPlan P = zrt::plan_launch(zrt::shape_of(h), params);
    // (as zrt_ctx_render_tiles decides)
    *lean = zrt::lean_launch(P, (params->flags & ZRT_FLAG_STATS) != 0,
                             zrt::camera_inside(camera, h.root_c, h.origin_bound))
                ? 1u
                : 0u;
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_tile_classes(const zrt_scene* scene, const zrt_camera* camera, const zrt_params* params,
                           uint32_t* classes, uint32_t cap, uint32_t* n_tiles, uint32_t* n_sky, double* margins) {
  if (!camera || !n_tiles || !n_sky || (cap && !classes)) return fail(ZRT_E_INVALID, "null argument");
  *n_tiles = *n_sky = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  rc = zrt::validate_params(params);
  if (rc) return rc;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;  // (zrt_ctx_create)
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, use_bvh, -1);
    const zrt::LaunchPlan P = zrt::plan_launch(zrt::shape_of(h), params);
    std::vector<uint32_t> cls(zrt::rank_tiles(zrt::geometry(params), params->rank, params->world_size), zrt::kTileGeneral);
    if (margins) margins[0] = margins[1] = margins[2] = margins[3] = 0.0;
    // (as zrt_ctx_render_tiles decides)
    if (zrt::sky_tiles_wanted() &&
        zrt::sky_split_allowed(P, params, zrt::camera_inside(camera, h.root_c, h.origin_bound))) {
      zrt::SkyScene sky;
      zrt::build_sky_scene(&sky, h);
      const double t0 = zrt::now_ms();
      zrt::OneSphere one;
      one.want = zrt::sphere_tiles_wanted() &&
                 zrt::sphere_split_allowed(P, params, zrt::camera_inside(camera, h.root_c, h.origin_bound));
      zrt::classify_tiles(sky, camera, params, &cls, n_sky, margins, &one);
      if (std::getenv("ZRT_DEBUG_LAUNCH"))
        std::fprintf(stderr, "zrt tile classes: %u sky, %u one-sphere of %zu tiles in %.2f ms\n", *n_sky, one.n_tiles,
                     cls.size(), zrt::now_ms() - t0);
    }
    *n_tiles = uint32_t(cls.size());
    for (uint32_t i = 0; i < cap && i < cls.size(); ++i) classes[i] = cls[i];
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_slot_prims(const zrt_scene* scene, const zrt_params* params, uint32_t* prims, uint32_t cap,
                         uint32_t* n_slots) {
  if (!n_slots || (cap && !prims)) return fail(ZRT_E_INVALID, "null argument");
  *n_slots = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  rc = zrt::validate_params(params);
  if (rc) return rc;
  try {
    const bool use_bvh = params->bounded_volume_hierarchy != 0 && scene->n_prims > 10;  // (zrt_ctx_create)
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, use_bvh, -1);
    *n_slots = uint32_t(h.slot_to_prim.size());
    for (uint32_t i = 0; i < cap && i < h.slot_to_prim.size(); ++i) prims[i] = h.slot_to_prim[i];
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}

int zrt_debug_qnodes(const zrt_scene* scene, uint64_t* n_checked) {
  if (!n_checked) return fail(ZRT_E_INVALID, "null argument");
  *n_checked = 0;
  int rc = zrt::validate_scene(scene);
  if (rc) return rc;
  if (scene->n_prims <= 10) return fail(ZRT_E_INVALID, "no BVH for <= 10 surfaces (raytrace.zig:124-133)");
  try {
    zrt::HostScene h;
    zrt::flatten_scene(&h, scene, true, -1, 1);  // (the compressed nodes asked for explicitly)
    if (!h.q_ok) return fail(ZRT_E_UNSUPPORTED, "the encoder refused this tree (a non-finite plane)");
    const uint32_t nn = h.q_stride / zrt::kQuantNodeF4, nw = h.wide_stride / 8u;
    if (nn != nw) return fail(ZRT_E_UNSUPPORTED, "compressed and full trees differ in node count");
    auto bad = [](const std::string& what, uint32_t o, uint32_t i, int k) {
      return fail(ZRT_E_UNSUPPORTED, what + " (octant " + std::to_string(o) + ", node " + std::to_string(i) + ", slot " +
                                         std::to_string(k) + ")");
    };
    for (uint32_t o = 0; o < 8; ++o) {
      for (uint32_t i = 0; i < nn; ++i) {
        const float4* F = &h.wn[size_t(o) * h.wide_stride + 8u * i];  // full node, this octant's copy
        uint32_t W[16];
        std::memcpy(W, &h.qn[size_t(o) * h.q_stride + zrt::kQuantNodeF4 * i], sizeof(W));
        float org[3], step[3];
        std::memcpy(org, W, 12);
        for (int a = 0; a < 3; ++a) step[a] = std::ldexp(1.0f, int((W[3] >> (8 * a)) & 0xffu) - 127);
        int32_t fr[4], qr[4], fb[4];
        std::memcpy(fr, &F[6], 16);
        std::memcpy(fb, &F[7], 16);
        std::memcpy(qr, &W[10], 16);
        for (int k = 0; k < 4; ++k) {
          const float* fn = reinterpret_cast<const float*>(F);
          const bool empty = qr[k] == zrt::kEmptyRef;
          for (int a = 0; a < 3 && !empty; ++a) {
            const double qn = double((W[4 + a] >> (8 * k)) & 0xffu), qf = double((W[7 + a] >> (8 * k)) & 0xffu);
            const double dn = double(org[a]) + qn * double(step[a]), df = double(org[a]) + qf * double(step[a]);
            if (double(float(dn)) != dn || double(float(df)) != df) return bad("a plane does not decode exactly", o, i, k);
            const bool neg = (o >> a) & 1u;  // the near plane is the max one
            const double full_n = fn[4 * a + k], full_f = fn[4 * (3 + a) + k];
            if (neg ? !(dn >= full_n && df <= full_f) : !(dn <= full_n && df >= full_f))
              return bad("a decoded box does not contain the full node's", o, i, k);
          }
          if (!empty && qr[k] >= 0 && qr[k] != fr[k]) return bad("an inner child ref differs", o, i, k);
          if (!empty && qr[k] < 0) {
            const bool sph = qr[k] < -zrt::kSphereSlotBias;
            const uint32_t L = uint32_t(-(sph ? qr[k] + zrt::kSphereSlotBias : qr[k]) - 1);
            if (size_t(L) * zrt::kLeafRecF4 + 1 >= h.ql.size()) return bad("a leaf record index past the records", o, i, k);
            const float4 mn = h.ql[zrt::kLeafRecF4 * size_t(L)], mx = h.ql[zrt::kLeafRecF4 * size_t(L) + 1];
            const float m[3] = {mn.x, mn.y, mn.z}, M[3] = {mx.x, mx.y, mx.z};
            for (int a = 0; a < 3; ++a) {
              const bool neg = (o >> a) & 1u;
              const float full_n = fn[4 * a + k], full_f = fn[4 * (3 + a) + k];
              const float rn = neg ? M[a] : m[a], rf = neg ? m[a] : M[a];
              if (std::memcmp(&rn, &full_n, 4) || std::memcmp(&rf, &full_f, 4)) return bad("a leaf record's box differs", o, i, k);
            }
            int32_t ra, rb;
            std::memcpy(&ra, &mn.w, 4);
            std::memcpy(&rb, &mx.w, 4);
            const int32_t full_a = sph ? fr[k] + zrt::kSphereSlotBias : fr[k];
            if (ra != full_a || rb != fb[k] || sph != (fr[k] < -zrt::kSphereSlotBias))
              return bad("a leaf record's refs differ", o, i, k);
          }
          ++*n_checked;
        }
      }
    }
    return ZRT_OK;
  }
  ZRT_CATCH_HOST
}
