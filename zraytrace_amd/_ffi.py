"""ctypes view of include/zrt.h (the C ABI of libzrt.so).

The structures mirror the header field for field; `load()` opens the in-tree
``zraytrace_amd/libzrt.so`` built by ``__graft_entry__.build()`` and fails
loudly when it is missing: there is no Python or CPU fallback for the HIP path.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# ZRT_LIB overrides the library path (A/B of build variants, tools/variants.sh)
LIB_PATH = os.environ.get("ZRT_LIB") or os.path.join(HERE, "libzrt.so")

# ---- status / enums (zrt.h) --------------------------------------------------
ABI_VERSION = 2  # ZRT_ABI_VERSION: the layouts below (zrt_stats gained sampling_loop in 2)
ZRT_OK = 0
ZRT_E_INVALID = -1
ZRT_E_NOMEM = -2
ZRT_E_HIP = -3
ZRT_E_UNSUPPORTED = -4
ZRT_E_NODEVICE = -5
ZRT_E_IO = -6
ZRT_E_PARSE = -7

ZRT_PRIM_SPHERE, ZRT_PRIM_TRIANGLE = 0, 1
ZRT_MAT_LAMBERTIAN, ZRT_MAT_METAL, ZRT_MAT_DIELECTRIC = 0, 1, 2
ZRT_TEX_COLOR, ZRT_TEX_IMAGE = 0, 1
ZRT_RNG_COUNTER, ZRT_RNG_REFERENCE_STREAM = 0, 1
ZRT_PRNG_XOROSHIRO128, ZRT_PRNG_XOSHIRO256 = 0, 1
ZRT_TRAVERSAL_FAST, ZRT_TRAVERSAL_REFERENCE, ZRT_TRAVERSAL_BINARY = 0, 1, 2
ZRT_FLAG_STATS = 1
ZRT_FLAG_NO_SCHEDULE = 2
ZRT_FLAG_SCANLINES = 4
ZRT_FLAG_GUARD = 8
ZRT_DN_DEMODULATE = 1
ZRT_TA_DEMODULATE = 1
ZRT_AO_ACCUMULATE = 1
ZRT_AO_REDUCE_WAVE, ZRT_AO_REDUCE_ATOMIC = 0, 1
ZRT_RQ_ACCUMULATE = 1
ZRT_CQ_ACCUMULATE = 1
ZRT_LENS_PINHOLE, ZRT_LENS_THIN, ZRT_LENS_ORTHO, ZRT_LENS_EQUIRECT, ZRT_LENS_FISHEYE = range(5)


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class Camera(C.Structure):
    _fields_ = [("origin", Vec3), ("lower_left_corner", Vec3),
                ("horizontal", Vec3), ("vertical", Vec3)]


class Prim(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("material", C.c_uint32), ("center", Vec3),
                ("radius", C.c_float), ("a", Vec3), ("b", Vec3), ("c", Vec3)]


class Material(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("texture", C.c_uint32),
                ("index_of_refraction", C.c_float)]


class Texture(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("image", C.c_uint32), ("color", Vec3),
                ("u_offset", C.c_float), ("v_offset", C.c_float)]


class Image(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32),
                ("pixels", C.POINTER(C.c_float))]


class Scene(C.Structure):
    _fields_ = [("prims", C.POINTER(Prim)), ("n_prims", C.c_uint32),
                ("n_materials", C.c_uint32), ("materials", C.POINTER(Material)),
                ("textures", C.POINTER(Texture)), ("n_textures", C.c_uint32),
                ("n_images", C.c_uint32), ("images", C.POINTER(Image))]


class Params(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32),
                ("samples_per_pixel", C.c_uint32), ("max_depth", C.c_uint32),
                ("bounded_volume_hierarchy", C.c_uint32), ("rng_mode", C.c_uint32),
                ("prng", C.c_uint32), ("traversal", C.c_uint32), ("seed", C.c_uint64),
                ("rank", C.c_uint32), ("world_size", C.c_uint32),
                ("device", C.c_uint32), ("sample_chunk", C.c_uint32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("recursion_depth_hits", C.c_uint64), ("reflections", C.c_uint64),
                ("background_hits", C.c_uint64), ("pixels_processed", C.c_uint64),
                ("samples_processed", C.c_uint64), ("rays_processed", C.c_uint64),
                ("node_visits", C.c_uint64), ("prim_tests", C.c_uint64),
                ("sphere_tests", C.c_uint64), ("shade_fetches", C.c_uint64),
                ("texel_fetches", C.c_uint64), ("leaf_visits", C.c_uint64),
                ("preprocess_ms", C.c_double), ("upload_ms", C.c_double),
                ("render_ms", C.c_double), ("gather_ms", C.c_double),
                ("used_bvh", C.c_uint32), ("bvh_nodes", C.c_uint32),
                ("bvh_max_depth", C.c_uint32), ("n_gpus", C.c_uint32),
                ("node_bytes", C.c_uint32), ("wide_nodes", C.c_uint32),
                ("texel_bytes", C.c_uint32), ("schedule_ms", C.c_float),
                ("order_replays", C.c_uint64), ("box_excess_max_triangle", C.c_float),
                ("box_excess_max_sphere", C.c_float), ("box_excess_hits", C.c_uint64),
                ("sampling_loop", C.c_uint32), ("guard", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class Scanline(C.Structure):
    _fields_ = [("recursion_depth_hits", C.c_uint64), ("reflections", C.c_uint64),
                ("background_hits", C.c_uint64), ("pixels", C.c_uint64), ("samples", C.c_uint64),
                ("rays", C.c_uint64)]


SCANLINE_FIELDS = [name for name, _ in Scanline._fields_]


class LaunchPlan(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("kmode", C.c_uint32), ("sampling_loop", C.c_uint32),
                ("stk16", C.c_uint32), ("wf", C.c_uint32), ("pool", C.c_uint32), ("qnodes", C.c_uint32),
                ("guard_on", C.c_uint32), ("stack_depth", C.c_uint32), ("stack_rows", C.c_uint32),
                ("att_rows", C.c_uint32), ("att_rows_per_path", C.c_uint32), ("mats_in_lds", C.c_uint32),
                ("lds_bytes", C.c_uint32), ("ovf_bytes_per_lane", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class PassInfo(C.Structure):
    _fields_ = [("samples_done", C.c_uint32), ("pass_samples", C.c_uint32), ("changed_pixels", C.c_uint64),
                ("max_abs_change", C.c_float), ("render_ms", C.c_float), ("schedule_ms", C.c_float),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class PassPlan(C.Structure):
    _fields_ = [("first_sample", C.c_uint32), ("pass_samples", C.c_uint32), ("samples_after", C.c_uint32),
                ("chunk", C.c_uint32), ("pass_chunks", C.c_uint32), ("last_chunk", C.c_uint32),
                ("partial_bytes", C.c_uint64), ("key_offset", C.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


# zrt_pass_fn: int (*)(void* user, const float* rgb, const zrt_pass_info* info)
PASS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(PassInfo))


class Adaptive(C.Structure):
    _fields_ = [("tolerance", C.c_float), ("first_level", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class LevelInfo(C.Structure):
    _fields_ = [("level_samples", C.c_uint32), ("tiles_rendered", C.c_uint32), ("tiles_active_after", C.c_uint32),
                ("reserved", C.c_uint32), ("samples_rendered", C.c_uint64), ("changed_pixels", C.c_uint64),
                ("max_abs_change", C.c_float), ("render_ms", C.c_float), ("schedule_ms", C.c_float),
                ("reserved2", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if not name.startswith("reserved")}


# zrt_level_fn: int (*)(void* user, const float* rgb, const zrt_level_info* info)
LEVEL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.POINTER(LevelInfo))


class Denoise(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_albedo", C.c_float), ("sigma_depth", C.c_float), ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class VariancePlan(C.Structure):
    _fields_ = [("chunk", C.c_uint32), ("k", C.c_uint32), ("ik", C.c_float), ("sc", C.c_float)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class ReprojectPlan(C.Structure):
    _fields_ = [("origin", Vec3), ("rn", Vec3), ("ru", Vec3), ("rv", Vec3), ("s", C.c_float), ("valid", C.c_uint32)]


class Temporal(C.Structure):
    _fields_ = [("alpha_min", C.c_float), ("max_history", C.c_uint32), ("sigma_normal", C.c_float),
                ("sigma_depth", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


# zrt_frame_fn: int (*)(void* user, const float* rgb, uint32_t frame)
FRAME_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_float), C.c_uint32)


class Ao(C.Structure):
    _fields_ = [("n_samples", C.c_uint32), ("first_sample", C.c_uint32), ("radius", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class AoPlan(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("groups", C.c_uint64), ("pixel_slots", C.c_uint64),
                ("resident_lanes", C.c_uint64), ("ovf_row_bytes", C.c_uint64), ("plane_bytes", C.c_uint64),
                ("grid", C.c_uint32), ("blocks_per_cu", C.c_uint32), ("reduction", C.c_uint32),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class Radiance(C.Structure):
    _fields_ = [("n_samples", C.c_uint32), ("first_sample", C.c_uint32), ("first_ray", C.c_uint64),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RadianceInfo(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("rays", C.c_uint64), ("reflections", C.c_uint64),
                ("background_hits", C.c_uint64), ("recursion_depth_hits", C.c_uint64), ("kernel_ms", C.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class RadiancePlan(C.Structure):
    _fields_ = [("items", C.c_uint64), ("partial_bytes", C.c_uint64), ("resident_lanes", C.c_uint64),
                ("key_offset", C.c_uint64), ("chunk", C.c_uint32), ("call_chunks", C.c_uint32),
                ("last_chunk", C.c_uint32), ("chunks_per_round", C.c_uint32), ("rounds", C.c_uint32),
                ("grid", C.c_uint32), ("blocks_per_cu", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "reserved"}


class Lens(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("origin", Vec3), ("lower_left_corner", Vec3), ("horizontal", Vec3),
                ("vertical", Vec3), ("axis_u", Vec3), ("axis_v", Vec3), ("axis_w", Vec3), ("half_fov", C.c_float),
                ("reserved", C.c_uint32 * 2)]


class CameraQuery(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32),
                ("n_samples", C.c_uint32), ("first_sample", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 5)]


class Rect(C.Structure):
    _fields_ = [("x0", C.c_uint32), ("y0", C.c_uint32), ("w", C.c_uint32), ("h", C.c_uint32)]


class CameraPlan(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("pixels", C.c_uint64), ("tiles_w", C.c_uint32), ("tiles_h", C.c_uint32),
                ("radiance", RadiancePlan)]

    def as_dict(self):
        return {"slots": self.slots, "pixels": self.pixels, "tiles_w": self.tiles_w, "tiles_h": self.tiles_h,
                "radiance": self.radiance.as_dict()}


class BvhNode(C.Structure):
    _fields_ = [("min", Vec3), ("left", C.c_int32), ("max", Vec3), ("right", C.c_int32)]


# Every symbol include/zrt.h declares: (name, restype, argtypes)
_P = C.c_void_p
SIGNATURES = [
    ("zrt_render", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                             C.POINTER(C.c_float), C.POINTER(Stats)]),
    ("zrt_render_progress", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                      C.POINTER(C.c_float), C.POINTER(Stats), C.POINTER(Scanline)]),
    ("zrt_render_multi", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                   C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_float), C.POINTER(Stats)]),
    ("zrt_multi_create", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(C.c_uint32), C.c_uint32,
                                   C.POINTER(_P)]),
    ("zrt_multi_render", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), C.POINTER(C.c_float),
                                   C.POINTER(Stats)]),
    ("zrt_multi_destroy", C.c_int, [_P]),
    ("zrt_multi_scanlines", C.c_int, [_P, C.POINTER(Scanline), C.c_uint32]),
    ("zrt_multi_frame", C.c_int, [_P, C.POINTER(C.c_float), C.c_uint64]),
    ("zrt_multi_rank_ms", C.c_int, [_P, C.POINTER(C.c_double), C.c_uint32]),
    ("zrt_trace", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(C.c_float), C.c_uint32,
                            C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    ("zrt_camera_init", C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float),
                                  C.POINTER(C.c_float), C.c_float, C.c_float,
                                  C.POINTER(Camera)]),
    ("zrt_last_error", C.c_char_p, []),
    ("zrt_abi_version", C.c_int, []),
    ("zrt_build_info", C.c_char_p, []),
    ("zrt_build_id", C.c_char_p, []),
    ("zrt_ctx_create", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(_P)]),
    ("zrt_ctx_destroy", C.c_int, [_P]),
    ("zrt_ctx_tile_count", C.c_int, [_P, C.POINTER(Params), C.POINTER(C.c_uint32)]),
    ("zrt_ctx_render_tiles", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), _P, _P]),
    ("zrt_ctx_assemble", C.c_int, [_P, C.POINTER(Params), _P, _P, _P]),
    ("zrt_ctx_assemble_padded", C.c_int, [_P, C.POINTER(Params), _P, C.c_uint32, _P, _P]),
    ("zrt_ctx_sync", C.c_int, [_P]),
    ("zrt_ctx_scanlines", C.c_int, [_P, C.POINTER(Scanline), C.c_uint32]),
    ("zrt_ctx_stats", C.c_int, [_P, C.POINTER(Stats)]),
    ("zrt_ctx_last_kernel_ms", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("zrt_ctx_debug_counters", C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint32]),
    ("zrt_ctx_debug_wave_times", C.c_int, [_P, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    ("zrt_ctx_debug_schedule", C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32,
                                         C.POINTER(C.c_uint32)]),
    ("zrt_ctx_accum_begin", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params)]),
    ("zrt_ctx_accum_pass", C.c_int, [_P, C.c_uint32, _P, _P]),
    ("zrt_ctx_accum_info", C.c_int, [_P, C.POINTER(PassInfo)]),
    ("zrt_render_progressive", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.c_uint32,
                                         PASS_FN, _P, C.POINTER(C.c_float), C.POINTER(Stats)]),
    ("zrt_debug_pass_plan", C.c_int, [C.POINTER(Params), C.c_uint32, C.c_uint32, C.POINTER(PassPlan)]),
    ("zrt_ctx_adapt_begin", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), C.POINTER(Adaptive)]),
    ("zrt_ctx_adapt_level", C.c_int, [_P, _P, _P, C.POINTER(LevelInfo)]),
    ("zrt_ctx_adapt_samples", C.c_int, [_P, C.POINTER(C.c_uint32), C.c_uint32]),
    ("zrt_render_adaptive", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.POINTER(Adaptive),
                                      LEVEL_FN, _P, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(Stats)]),
    ("zrt_render_adaptive_progress", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                               C.POINTER(Adaptive), LEVEL_FN, _P, C.POINTER(C.c_float),
                                               C.POINTER(C.c_uint32), C.POINTER(Stats), C.POINTER(Scanline)]),
    ("zrt_debug_adapt_plan", C.c_int, [C.POINTER(Params), C.POINTER(Adaptive), C.POINTER(C.c_uint32), C.c_uint32,
                                       C.POINTER(C.c_uint32)]),
    ("zrt_ctx_features", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), _P, _P]),
    ("zrt_render_denoised", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.POINTER(Adaptive),
                                      C.POINTER(Denoise), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.POINTER(Stats), C.POINTER(C.c_double)]),
    ("zrt_denoise_defaults", C.c_int, [C.POINTER(Denoise)]),
    ("zrt_ctx_denoise", C.c_int, [_P, C.POINTER(Params), C.POINTER(Denoise), _P, _P, _P, _P]),
    ("zrt_ctx_denoise_ms", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("zrt_ctx_accum_variance", C.c_int, [_P, _P, _P]),
    ("zrt_ctx_assemble_plane", C.c_int, [_P, C.POINTER(Params), _P, C.c_uint32, _P, _P]),
    ("zrt_debug_variance_plan", C.c_int, [C.POINTER(Params), C.c_uint32, C.POINTER(VariancePlan)]),
    ("zrt_denoise_guided_defaults", C.c_int, [C.POINTER(Denoise), C.POINTER(C.c_uint32)]),
    ("zrt_ctx_denoise_guided", C.c_int, [_P, C.POINTER(Params), C.POINTER(Denoise), C.c_uint32, _P, _P, _P, _P, _P,
                                         _P]),
    ("zrt_render_denoised_guided", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                             C.POINTER(Adaptive), C.POINTER(Denoise), C.c_uint32,
                                             C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                             C.POINTER(C.c_float), C.POINTER(Stats), C.POINTER(C.c_double)]),
    ("zrt_debug_reproject_plan", C.c_int, [C.POINTER(Camera), C.POINTER(Params), C.POINTER(ReprojectPlan)]),
    ("zrt_temporal_defaults", C.c_int, [C.POINTER(Temporal)]),
    ("zrt_ctx_temporal", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), C.POINTER(Temporal), _P, _P, _P, _P, _P,
                                   _P, _P]),
    ("zrt_ctx_temporal_reset", C.c_int, [_P]),
    ("zrt_ctx_temporal_ms", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("zrt_render_temporal", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.c_uint32, C.POINTER(Params),
                                      C.POINTER(Temporal), C.POINTER(Denoise), C.c_uint32, FRAME_FN, _P,
                                      C.POINTER(C.c_float), C.POINTER(Stats)]),
    ("zrt_ctx_trace", C.c_int, [_P, C.POINTER(Params), _P, C.c_uint32, _P, _P, _P]),
    ("zrt_ctx_occluded", C.c_int, [_P, C.POINTER(Params), _P, _P, C.c_uint32, _P, _P]),
    ("zrt_occluded", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(C.c_float), C.POINTER(C.c_float),
                               C.c_uint32, C.POINTER(C.c_uint8)]),
    ("zrt_ctx_query_ms", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("zrt_ctx_ao", C.c_int, [_P, C.POINTER(Camera), C.POINTER(Params), C.POINTER(Ao), _P, _P, _P, _P]),
    ("zrt_ctx_ao_ms", C.c_int, [_P, C.POINTER(C.c_double)]),
    ("zrt_render_ao", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params), C.POINTER(Ao),
                                C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    ("zrt_debug_ao_plan", C.c_int, [C.POINTER(Params), C.POINTER(Ao), C.c_uint32, C.POINTER(AoPlan)]),
    ("zrt_ctx_radiance", C.c_int, [_P, C.POINTER(Params), C.POINTER(Radiance), _P, C.c_uint32, _P, _P, _P]),
    ("zrt_ctx_radiance_info", C.c_int, [_P, C.POINTER(RadianceInfo)]),
    ("zrt_ctx_debug_radiance", C.c_int, [_P, C.POINTER(C.c_uint32)]),
    ("zrt_radiance", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(Radiance), C.POINTER(C.c_float),
                               C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(RadianceInfo)]),
    ("zrt_debug_radiance_plan", C.c_int, [C.POINTER(Params), C.POINTER(Radiance), C.c_uint32, C.c_uint32, C.c_uint64,
                                          C.POINTER(RadiancePlan)]),
    ("zrt_rays_equirect", C.c_int, [C.POINTER(C.c_float), C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    ("zrt_ctx_camera", C.c_int, [_P, C.POINTER(Params), C.POINTER(Lens), C.POINTER(CameraQuery), _P, _P, _P]),
    ("zrt_ctx_camera_info", C.c_int, [_P, C.POINTER(RadianceInfo)]),
    ("zrt_render_lens", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(Lens), C.POINTER(CameraQuery),
                                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(RadianceInfo)]),
    ("zrt_debug_camera_plan", C.c_int, [C.POINTER(Params), C.POINTER(CameraQuery), C.c_uint32, C.c_uint64,
                                        C.POINTER(CameraPlan)]),
    ("zrt_lens_check", C.c_int, [C.POINTER(Lens)]),
    ("zrt_rect_check", C.c_int, [C.POINTER(Params), C.POINTER(Rect)]),
    ("zrt_ctx_camera_features", C.c_int, [_P, C.POINTER(Params), C.POINTER(Lens), C.POINTER(Rect), _P, _P]),
    ("zrt_ctx_camera_moments", C.c_int, [_P, C.POINTER(Params), C.POINTER(Lens), C.POINTER(CameraQuery), _P, _P,
                                         _P]),
    ("zrt_ctx_camera_variance", C.c_int, [_P, C.POINTER(Params), C.POINTER(Rect), C.c_uint32, _P, _P, _P]),
    ("zrt_ctx_denoise_rect", C.c_int, [_P, C.POINTER(Params), C.POINTER(Denoise), C.c_uint32, C.POINTER(Rect), _P, _P,
                                       _P, _P, _P, _P]),
    ("zrt_render_lens_denoised", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(Lens),
                                           C.POINTER(CameraQuery), C.POINTER(Denoise), C.c_uint32, C.c_uint32,
                                           C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                           C.POINTER(C.c_float), C.POINTER(RadianceInfo), C.POINTER(C.c_double)]),
    ("zrt_lens_init", C.c_int, [C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.POINTER(Lens)]),
    ("zrt_lens_from_camera", C.c_int, [C.c_uint32, C.POINTER(Camera), C.c_float, C.c_float, C.c_float,
                                       C.POINTER(Lens)]),
    ("zrt_scene_load", C.c_int, [C.c_uint32, C.c_char_p, C.POINTER(_P), C.POINTER(Camera)]),
    ("zrt_scene_view", C.POINTER(Scene), [_P]),
    ("zrt_scene_free", None, [_P]),
    ("zrt_scene_write", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.c_char_p]),
    ("zrt_scene_read", C.c_int, [C.c_char_p, C.POINTER(_P), C.POINTER(Camera)]),
    ("zrt_obj_read", C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(C.POINTER(Prim)),
                               C.POINTER(C.c_uint32)]),
    ("zrt_free", None, [_P]),
    ("zrt_image_read_png", C.c_int, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                     C.POINTER(C.POINTER(C.c_float))]),
    ("zrt_image_write_png", C.c_int, [C.c_char_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32]),
    ("zrt_image_write_ppm", C.c_int, [C.c_char_p, C.POINTER(C.c_float), C.c_uint32, C.c_uint32]),
    ("zrt_bvh_build", C.c_int, [C.POINTER(Scene), C.POINTER(C.POINTER(BvhNode)),
                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("zrt_bvh_build_device", C.c_int, [C.POINTER(Scene), C.c_uint32, C.POINTER(C.POINTER(BvhNode)),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("zrt_debug_math", C.c_int, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 C.POINTER(C.c_float), C.c_uint32, C.c_uint32]),
    ("zrt_debug_rng", C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64),
                                C.c_uint32, C.c_uint32]),
    ("zrt_debug_division", C.c_int, [C.c_uint64, C.POINTER(C.c_uint64), C.c_uint32]),
    ("zrt_debug_compact", C.c_int, [C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32,
                                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_uint32]),
    ("zrt_debug_lds_plans", C.c_int, [C.POINTER(Scene), C.POINTER(C.c_uint32)]),
    ("zrt_debug_buffer_plans", C.c_int, [C.POINTER(Scene), C.c_uint32, C.POINTER(C.c_uint32)]),
    ("zrt_debug_launch_plan", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(LaunchPlan)]),
    ("zrt_debug_lean_kernel", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                        C.POINTER(C.c_uint32)]),
    ("zrt_debug_qnodes", C.c_int, [C.POINTER(Scene), C.POINTER(C.c_uint64)]),
    ("zrt_debug_tile_classes", C.c_int, [C.POINTER(Scene), C.POINTER(Camera), C.POINTER(Params),
                                         C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_double)]),
    ("zrt_debug_octant_offsets", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32]),
    ("zrt_debug_slot_prims", C.c_int, [C.POINTER(Scene), C.POINTER(Params), C.POINTER(C.c_uint32), C.c_uint32,
                                       C.POINTER(C.c_uint32)]),
]

_lib = None


class ZrtError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"zrt error {code}: {msg}")
        self.code = code


def load(path: str = LIB_PATH):
    """Open libzrt.so (the HIP path).  Raises if it was not built."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    # One HIP runtime per process: libzrt.so and torch both NEED
    # libamdhip64.so.7, and torch ships its own copy (with its own HSA runtime).
    # Whichever is loaded first is the one the process uses, and a second HSA
    # runtime cannot open the GPU.  Load torch's first so device buffers, streams
    # and RCCL (torch.distributed) share the runtime libzrt launches on.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'); there is no fallback path")
    lib = C.CDLL(path)
    in_tree = path == os.path.join(HERE, "libzrt.so")
    rebuild = "rebuild it (python -c 'import __graft_entry__ as g; g.build()')"
    # the ABI version first (every version exports zrt_abi_version): the struct
    # layouts below are this version's, so another version is refused before any
    # symbol is bound - an A/B variant under ZRT_LIB too (its Params / Stats would be
    # read with this version's layouts), unless ZRT_ALLOW_ABI_MISMATCH=1 asks for it
    lib.zrt_abi_version.restype = C.c_int
    lib.zrt_abi_version.argtypes = []
    abi = lib.zrt_abi_version()
    if abi != ABI_VERSION:
        if in_tree:
            raise ImportError(f"{path} has ABI version {abi}, this binding expects {ABI_VERSION}: {rebuild}")
        if os.environ.get("ZRT_ALLOW_ABI_MISMATCH") != "1":
            raise ImportError(f"ZRT_LIB {path} has ABI version {abi}, this binding expects {ABI_VERSION} "
                              "(set ZRT_ALLOW_ABI_MISMATCH=1 to bind it anyway)")
        import warnings
        warnings.warn(f"ZRT_LIB {path} has ABI version {abi}, this binding expects {ABI_VERSION} "
                      "(bound anyway: ZRT_ALLOW_ABI_MISMATCH=1)")
    for name, restype, argtypes in SIGNATURES:
        if not hasattr(lib, name):
            if in_tree:
                raise ImportError(f"{path} does not export {name} (built from older sources): {rebuild}")
            continue  # an older A/B build variant (ZRT_LIB) may lack newer entry points
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if path == LIB_PATH:
        _lib = lib
    return lib


def check(rc: int):
    if rc != ZRT_OK:
        raise ZrtError(rc, (load().zrt_last_error() or b"").decode())
    return rc
