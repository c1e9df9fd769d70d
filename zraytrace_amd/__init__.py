"""zraytrace_amd — MI355X (gfx950) path of zraytrace's per-pixel sampling loop.

Python host helpers over the C ABI (include/zrt.h, libzrt.so).  The reference
names carry over: ``render`` replaces raytrace.render (raytrace.zig:136-203),
``load_scene`` builds the scenes of scenes.zig:267-277 (through the C++ host
mirror in csrc/scene_io.cpp), ``RenderParams`` mirrors raytrace.zig:102-108.

There is no CPU fallback: every call that renders goes through the HIP kernel
in libzrt.so and raises ZrtError(ZRT_E_NODEVICE) without an MI355X.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import _ffi
from ._ffi import (ZRT_PRNG_XOROSHIRO128, ZRT_PRNG_XOSHIRO256, ZRT_RNG_COUNTER,  # noqa: F401
                   ZRT_RNG_REFERENCE_STREAM, ZRT_TRAVERSAL_FAST, ZRT_TRAVERSAL_REFERENCE,
                   ZRT_TRAVERSAL_BINARY, ZRT_FLAG_STATS, ZRT_FLAG_NO_SCHEDULE, ZRT_FLAG_SCANLINES, ZRT_FLAG_GUARD,
                   ZRT_DN_DEMODULATE, ZRT_TA_DEMODULATE, ZRT_AO_ACCUMULATE, ZRT_AO_REDUCE_WAVE, ZRT_AO_REDUCE_ATOMIC,
                   ZRT_RQ_ACCUMULATE, ZRT_CQ_ACCUMULATE, ZRT_LENS_PINHOLE, ZRT_LENS_THIN, ZRT_LENS_ORTHO,
                   ZRT_LENS_EQUIRECT, ZRT_LENS_FISHEYE, ZrtError, check)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(REPO, "assets")

SCENES = {0: "manAndBall", 1: "threeBalls", 2: "bunnyAndBall", 3: "teapotAndBall",
          4: "teapotAndBallCircle", 5: "goat"}


def lib():
    return _ffi.load()


def build_id() -> str:
    """zrt_build_id() of the loaded library: sha1 of the kernel sources (16 hex)
    - sha1 of the device compile flags (8)."""
    L = lib()
    if not hasattr(L, "zrt_build_id"):  # an A/B variant built from older sources (ZRT_LIB)
        return "unknown"
    return L.zrt_build_id().decode()


def build_id_of_sources() -> str:
    """The source half of zrt_build_id() recomputed from the files in the tree:
    differs from build_id()'s when libzrt.so is stale against its sources."""
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    # csrc/Makefile ID_SRC: every source of the directory in sorted order, then include/zrt.h
    for f in sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".hpp", ".cpp"))):
        with open(os.path.join(csrc, f), "rb") as fh:
            h.update(fh.read())
    with open(os.path.join(REPO, "include", "zrt.h"), "rb") as fh:
        h.update(fh.read())
    return h.hexdigest()[:16]


@dataclass
class RenderParams:
    """raytrace.zig:102-108 plus the knobs of the GPU path."""
    width: int
    height: int
    samples_per_pixel: int
    max_depth: int
    bounded_volume_hierarchy: bool = True
    seed: int = 42
    rng_mode: int = ZRT_RNG_COUNTER
    prng: int = ZRT_PRNG_XOROSHIRO128
    traversal: int = ZRT_TRAVERSAL_FAST
    rank: int = 0
    world_size: int = 1
    device: int = 0
    sample_chunk: int = 0
    flags: int = 0

    def abi(self) -> _ffi.Params:
        p = _ffi.Params()
        p.width, p.height = self.width, self.height
        p.samples_per_pixel, p.max_depth = self.samples_per_pixel, self.max_depth
        p.bounded_volume_hierarchy = 1 if self.bounded_volume_hierarchy else 0
        p.rng_mode, p.prng, p.traversal = self.rng_mode, self.prng, self.traversal
        p.seed = self.seed
        p.rank, p.world_size, p.device = self.rank, self.world_size, self.device
        p.sample_chunk = self.sample_chunk
        p.flags = self.flags
        return p


class LoadedScene:
    """A scene of scenes.zig built by the C++ host mirror (zrt_scene_load), or
    read back from a binary scene file (zrt_scene_read, LoadedScene.read)."""

    def __init__(self, index: int, assets_dir: str = ASSETS, _path: str = None):
        L = lib()
        h = C.c_void_p()
        cam = _ffi.Camera()
        if _path is None:
            check(L.zrt_scene_load(index, assets_dir.encode(), C.byref(h), C.byref(cam)))
        else:
            check(L.zrt_scene_read(_path.encode(), C.byref(h), C.byref(cam)))
        self._h = h
        self.index = index
        self.camera = cam
        self.view = L.zrt_scene_view(h)  # POINTER(Scene)

    @classmethod
    def read(cls, path: str) -> "LoadedScene":
        """A scene written by write() (zrt_scene_read)."""
        return cls(-1, _path=path)

    def write(self, path: str):
        """The flat scene and its camera as a binary scene file (zrt_scene_write)."""
        check(lib().zrt_scene_write(self.view, C.byref(self.camera), path.encode()))

    @property
    def n_prims(self) -> int:
        return self.view.contents.n_prims

    def close(self):
        if getattr(self, "_h", None):
            lib().zrt_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_scene(index: int, assets_dir: str = ASSETS) -> LoadedScene:
    return LoadedScene(index, assets_dir)


def camera_init(look_from, look_at, vup, vfov, aspect) -> _ffi.Camera:
    """Camera.init (camera.zig:17-35)."""
    f3 = C.c_float * 3
    out = _ffi.Camera()
    check(lib().zrt_camera_init(f3(*look_from), f3(*look_at), f3(*vup), vfov, aspect, C.byref(out)))
    return out


def render(scene, camera: _ffi.Camera, params: RenderParams):
    """raytrace.render on the GPU: returns (image[H, W, 3] f32, row 0 = bottom; stats)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = _ffi.Stats()
    p = params.abi()
    check(lib().zrt_render(view, C.byref(camera), C.byref(p),
                           out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return out, st.as_dict()


def render_progressive(scene, camera: _ffi.Camera, params: RenderParams, pass_samples: int = 0, on_pass=None):
    """render() in passes of pass_samples samples (zrt_render_progressive; rounded up to
    whole sample chunks, 0: the library's default): returns (image, stats, [info dict
    per pass]).  on_pass(image[H, W, 3] so far, info dict) is called after every pass; a
    true return stops the run, and image / stats are then those of info["samples_done"]
    samples per pixel."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = _ffi.Stats()
    p = params.abi()
    infos = []

    def cb(_user, _rgb, info):
        infos.append(info.contents.as_dict())
        return 1 if on_pass is not None and on_pass(out, infos[-1]) else 0

    check(lib().zrt_render_progressive(view, C.byref(camera), C.byref(p), pass_samples, _ffi.PASS_FN(cb), None,
                                       out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return out, st.as_dict(), infos


def _adaptive(tolerance: float, first_level: int) -> _ffi.Adaptive:
    return _ffi.Adaptive(tolerance=tolerance, first_level=first_level)


def render_adaptive(scene, camera: _ffi.Camera, params: RenderParams, tolerance: float, first_level: int = 0,
                    on_level=None):
    """render() with adaptive sampling (zrt_render_adaptive; the rule: zrt.h): 8x8 tiles whose
    pixels all changed by no more than tolerance * sqrt(brightness) between two sample levels
    stop there.  Returns (image, samples uint32[H, W] per pixel, stats, [info dict per level]).
    on_level(image so far, info dict) is called after every level; a true return stops the run."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    samples = np.zeros((params.height, params.width), dtype=np.uint32)
    st = _ffi.Stats()
    p = params.abi()
    ad = _adaptive(tolerance, first_level)
    infos = []

    def cb(_user, _rgb, info):
        infos.append(info.contents.as_dict())
        return 1 if on_level is not None and on_level(out, infos[-1]) else 0

    check(lib().zrt_render_adaptive(view, C.byref(camera), C.byref(p), C.byref(ad), _ffi.LEVEL_FN(cb), None,
                                    out.ctypes.data_as(C.POINTER(C.c_float)),
                                    samples.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(st)))
    return out, samples, st.as_dict(), infos


def adapt_plan(params: RenderParams, tolerance: float, first_level: int = 0) -> list:
    """The sample levels of an adaptive run with these params (zrt_debug_adapt_plan; no
    device).  Raises ZrtError for what the run would refuse."""
    p = params.abi()
    ad = _adaptive(tolerance, first_level)
    levels = (C.c_uint32 * 32)()
    n = C.c_uint32()
    check(lib().zrt_debug_adapt_plan(C.byref(p), C.byref(ad), levels, 32, C.byref(n)))
    return list(levels[:n.value])


def debug_pass_plan(params: RenderParams, done: int, n_samples: int) -> dict:
    """How an accumulation run with these params (samples_per_pixel = its cap) renders
    samples [done, done + n_samples) (zrt_debug_pass_plan; no device): the zrt_pass_plan
    fields as a dict.  Raises ZrtError for a pass the run would refuse."""
    out = _ffi.PassPlan()
    p = params.abi()
    check(lib().zrt_debug_pass_plan(C.byref(p), done, n_samples, C.byref(out)))
    return out.as_dict()


def denoise_defaults() -> _ffi.Denoise:
    """The default a-trous filter (zrt_denoise_defaults; no device): iterations and the
    sigmas tools/denoise_probe.py's grid search chose."""
    out = _ffi.Denoise()
    check(lib().zrt_denoise_defaults(C.byref(out)))
    return out


def render_denoised(scene, camera: _ffi.Camera, params: RenderParams, tolerance: float = None, first_level: int = 0,
                    denoise: _ffi.Denoise = None):
    """render() (tolerance None) or render_adaptive(), then the first-hit feature buffers and
    the a-trous filter on the device (zrt_render_denoised; denoise None: the defaults).
    Returns (rgb: the denoised frame, noisy: the unfiltered one, features float32[H, W, 8]:
    {N.xyz, t, A.rgb, id bits}, stats); stats["denoise_ms"] is the filter's device time."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    f = C.POINTER(C.c_float)
    rgb = np.zeros((params.height, params.width, 3), dtype=np.float32)
    noisy = np.zeros((params.height, params.width, 3), dtype=np.float32)
    features = np.zeros((params.height, params.width, 8), dtype=np.float32)
    st = _ffi.Stats()
    ms = C.c_double()
    p = params.abi()
    ad = C.byref(_adaptive(tolerance, first_level)) if tolerance is not None else None
    dn = C.byref(denoise) if denoise is not None else None
    check(lib().zrt_render_denoised(view, C.byref(camera), C.byref(p), ad, dn, rgb.ctypes.data_as(f),
                                    noisy.ctypes.data_as(f), features.ctypes.data_as(f), C.byref(st), C.byref(ms)))
    stats = st.as_dict()
    stats["denoise_ms"] = ms.value
    return rgb, noisy, features, stats


def denoise_guided_defaults():
    """The default variance-guided filter (zrt_denoise_guided_defaults; no device): (the
    zrt_denoise tools/denoise_guided_probe.py's search chose, its flags)."""
    out = _ffi.Denoise()
    flags = C.c_uint32()
    check(lib().zrt_denoise_guided_defaults(C.byref(out), C.byref(flags)))
    return out, flags.value


def debug_variance_plan(params: RenderParams, n_samples: int) -> dict:
    """How the variance plane scales a pixel holding n_samples samples in chunks of
    params.sample_chunk (zrt_debug_variance_plan; no device): chunk, k, ik, sc.  Raises
    ZrtError for what zrt_ctx_accum_variance would refuse."""
    out = _ffi.VariancePlan()
    p = params.abi()
    check(lib().zrt_debug_variance_plan(C.byref(p), n_samples, C.byref(out)))
    return out.as_dict()


def render_denoised_guided(scene, camera: _ffi.Camera, params: RenderParams, tolerance: float = None,
                           first_level: int = 0, denoise: _ffi.Denoise = None, flags: int = None):
    """render_denoised() with the variance-guided filter (zrt_render_denoised_guided; denoise
    None: the guided defaults, flags None: their flags).  params.samples_per_pixel must be
    two or more whole sample chunks.  Returns (rgb, noisy, features, variance float32[H, W]:
    the noisy frame's variance plane, stats)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    f = C.POINTER(C.c_float)
    rgb = np.zeros((params.height, params.width, 3), dtype=np.float32)
    noisy = np.zeros((params.height, params.width, 3), dtype=np.float32)
    features = np.zeros((params.height, params.width, 8), dtype=np.float32)
    variance = np.zeros((params.height, params.width), dtype=np.float32)
    st = _ffi.Stats()
    ms = C.c_double()
    p = params.abi()
    ad = C.byref(_adaptive(tolerance, first_level)) if tolerance is not None else None
    if flags is None:
        flags = denoise_guided_defaults()[1]
    dn = C.byref(denoise) if denoise is not None else None
    check(lib().zrt_render_denoised_guided(view, C.byref(camera), C.byref(p), ad, dn, flags, rgb.ctypes.data_as(f),
                                           noisy.ctypes.data_as(f), features.ctypes.data_as(f),
                                           variance.ctypes.data_as(f), C.byref(st), C.byref(ms)))
    stats = st.as_dict()
    stats["denoise_ms"] = ms.value
    return rgb, noisy, features, variance, stats


def temporal_defaults() -> _ffi.Temporal:
    """The default temporal step (zrt_temporal_defaults; no device): what
    tools/temporal_probe.py's grid search chose."""
    out = _ffi.Temporal()
    check(lib().zrt_temporal_defaults(C.byref(out)))
    return out


def debug_reproject_plan(prev: _ffi.Camera, params: RenderParams) -> _ffi.ReprojectPlan:
    """The reprojection plan of a previous camera (zrt_debug_reproject_plan; no device)."""
    out = _ffi.ReprojectPlan()
    p = params.abi()
    check(lib().zrt_debug_reproject_plan(C.byref(prev), C.byref(p), C.byref(out)))
    return out


def render_temporal(scene, cameras, params: RenderParams, temporal: _ffi.Temporal = None,
                    denoise: _ffi.Denoise = None, flags: int = None, on_frame=None):
    """A sequence of frames, cameras[k] the camera of frame k, through the temporal step
    and the guided filter (zrt_render_temporal; temporal None: temporal_defaults(), denoise
    None: the guided defaults, flags None: their flags).  on_frame(rgb float32[H, W, 3], k)
    is called with each filtered frame; a true return stops the sequence.  Returns (the
    last filtered frame, the last frame's stats)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    cams = (_ffi.Camera * len(cameras))(*cameras)
    rgb = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = _ffi.Stats()
    p = params.abi()
    if flags is None:
        flags = denoise_guided_defaults()[1]

    def cb(_user, ptr, k):
        return 1 if on_frame(rgb.copy(), k) else 0

    fn = _ffi.FRAME_FN(cb) if on_frame is not None else C.cast(None, _ffi.FRAME_FN)
    check(lib().zrt_render_temporal(view, cams, len(cameras), C.byref(p),
                                    C.byref(temporal) if temporal is not None else None,
                                    C.byref(denoise) if denoise is not None else None, flags, fn, None,
                                    rgb.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return rgb, st.as_dict()


def _scanlines_np(rows) -> np.ndarray:
    """zrt_scanline[height] -> uint64 array [height, 6] (columns: _ffi.SCANLINE_FIELDS)."""
    return np.ctypeslib.as_array(rows).view(np.uint64).reshape(len(rows), 6).copy()


def render_progress(scene, camera: _ffi.Camera, params: RenderParams):
    """render() plus the per-scanline Progress counters of raytrace.zig:184
    (zrt_render_progress): (image, stats, rows uint64[H, 6]: recursion-limit
    hits, reflections, background hits, pixels, samples, rays of each row)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = _ffi.Stats()
    rows = (_ffi.Scanline * params.height)()
    p = params.abi()
    check(lib().zrt_render_progress(view, C.byref(camera), C.byref(p),
                                    out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st), rows))
    return out, st.as_dict(), _scanlines_np(rows)


def render_multi(scene, camera: _ffi.Camera, params: RenderParams, devices):
    """raytrace.render over several GPUs from one process (zrt_render_multi): tiles
    dealt round-robin over `devices`, one RCCL gather to devices[0].  A device
    listed twice runs two ranks (gathered by device copies).  Same image as render()."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = np.zeros((params.height, params.width, 3), dtype=np.float32)
    st = _ffi.Stats()
    p = params.abi()
    devs = (C.c_uint32 * len(devices))(*devices)
    check(lib().zrt_render_multi(view, C.byref(camera), C.byref(p), devs, len(devices),
                                 out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(st)))
    return out, st.as_dict()


class MultiContext:
    """Persistent multi-GPU context (zrt_multi_*): scene on every device of the
    list, RCCL communicators created once; render() = zrt_render_multi's frame."""

    def __init__(self, scene, params: RenderParams, devices):
        view = scene.view if isinstance(scene, LoadedScene) else scene
        self._scene = scene
        h = C.c_void_p()
        p = params.abi()
        devs = (C.c_uint32 * len(devices))(*devices)
        check(lib().zrt_multi_create(view, C.byref(p), devs, len(devices), C.byref(h)))
        self._h = h
        self.n_ranks = len(devices)
        self._shape = None

    def render(self, camera, params: RenderParams, copy_out: bool = True):
        """One frame.  copy_out=False leaves it on devices[0] (read it with frame()):
        returns (None, stats)."""
        st = _ffi.Stats()
        p = params.abi()
        out = np.zeros((params.height, params.width, 3), dtype=np.float32) if copy_out else None
        ptr = out.ctypes.data_as(C.POINTER(C.c_float)) if copy_out else None
        check(lib().zrt_multi_render(self._h, C.byref(camera), C.byref(p), ptr, C.byref(st)))
        self._shape = (params.height, params.width, 3)
        return out, st.as_dict()

    def frame(self) -> np.ndarray:
        """The last frame, copied from devices[0] (zrt_multi_frame)."""
        out = np.zeros(self._shape, dtype=np.float32)
        check(lib().zrt_multi_frame(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out

    def rank_ms(self) -> list:
        """Each rank's render-kernel time of the last frame, ms (zrt_multi_rank_ms)."""
        out = (C.c_double * self.n_ranks)()
        check(lib().zrt_multi_rank_ms(self._h, out, self.n_ranks))
        return list(out)

    def scanlines(self, height: int) -> np.ndarray:
        """Per-scanline counters of the last render made with ZRT_FLAG_SCANLINES, summed over ranks."""
        rows = (_ffi.Scanline * height)()
        check(lib().zrt_multi_scanlines(self._h, rows, height))
        return _scanlines_np(rows)

    def close(self):
        if getattr(self, "_h", None):
            lib().zrt_multi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trace(scene, params: RenderParams, origins, directions):
    """Closest hit of each ray (zrt_trace): (t float32[n], +inf on a miss; prim int32[n], -1 on a miss)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    rays = np.ascontiguousarray(np.concatenate([np.asarray(origins, np.float32).reshape(-1, 3),
                                                np.asarray(directions, np.float32).reshape(-1, 3)], axis=1))
    n = rays.shape[0]
    t = np.empty(n, np.float32)
    prim = np.empty(n, np.int32)
    p = params.abi()
    check(lib().zrt_trace(view, C.byref(p), rays.ctypes.data_as(C.POINTER(C.c_float)), n,
                          t.ctypes.data_as(C.POINTER(C.c_float)), prim.ctypes.data_as(C.POINTER(C.c_int32))))
    return t, prim


def occluded(scene, params: RenderParams, origins, directions, t_max=None):
    """Any hit of each ray in (0.001, t_max) (zrt_occluded; the definition: zrt.h "ray queries"):
    bool[n].  t_max: float32[n], or None = +inf for every ray."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    rays = np.ascontiguousarray(np.concatenate([np.asarray(origins, np.float32).reshape(-1, 3),
                                                np.asarray(directions, np.float32).reshape(-1, 3)], axis=1))
    n = rays.shape[0]
    out = np.zeros(n, np.uint8)
    tm = None
    if t_max is not None:
        tm = np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, np.float32), (n,)))
    p = params.abi()
    check(lib().zrt_occluded(view, C.byref(p), rays.ctypes.data_as(C.POINTER(C.c_float)),
                             tm.ctypes.data_as(C.POINTER(C.c_float)) if tm is not None else None, n,
                             out.ctypes.data_as(C.POINTER(C.c_uint8))))
    return out != 0


def ao_settings(n_samples: int, radius: float = float("inf"), first_sample: int = 0, flags: int = 0) -> _ffi.Ao:
    """A zrt_ao: n_samples cosine rays per pixel of length radius, the pixel's samples
    first_sample .. ; flags: ZRT_AO_ACCUMULATE."""
    return _ffi.Ao(n_samples=n_samples, first_sample=first_sample, radius=radius, flags=flags)


def render_ao(scene, camera: _ffi.Camera, params: RenderParams, n_samples: int, radius: float = float("inf"),
              first_sample: int = 0):
    """The frame's ambient-occlusion plane (zrt_render_ao; the definition: zrt.h "ambient
    occlusion"): n_samples cosine rays of length radius from every first hit.  Returns (ao
    float32[H, W]: the share of rays that got away, clear uint32[H, W]: their count,
    features float32[H, W, 8])."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    ao = np.zeros((params.height, params.width), dtype=np.float32)
    clear = np.zeros((params.height, params.width), dtype=np.uint32)
    features = np.zeros((params.height, params.width, 8), dtype=np.float32)
    p = params.abi()
    a = ao_settings(n_samples, radius, first_sample)
    f = C.POINTER(C.c_float)
    check(lib().zrt_render_ao(view, C.byref(camera), C.byref(p), C.byref(a), ao.ctypes.data_as(f),
                              clear.ctypes.data_as(C.POINTER(C.c_uint32)), features.ctypes.data_as(f)))
    return ao, clear, features


def debug_ao_plan(params: RenderParams, ao: _ffi.Ao, cu_count: int = 256) -> dict:
    """How zrt_ctx_ao launches with these params and settings on a device of cu_count CUs
    (zrt_debug_ao_plan; no device): rays, groups, grid, resident lanes, overflow-row bytes
    and the reduction.  Raises ZrtError for what the call would refuse."""
    out = _ffi.AoPlan()
    p = params.abi()
    check(lib().zrt_debug_ao_plan(C.byref(p), C.byref(ao), cu_count, C.byref(out)))
    return out.as_dict()


def radiance_settings(n_samples: int, first_sample: int = 0, first_ray: int = 0, flags: int = 0) -> _ffi.Radiance:
    """A zrt_radiance: n_samples samples per ray, the ray's samples first_sample .. ; the
    call's ray 0 has index first_ray; flags: ZRT_RQ_ACCUMULATE."""
    return _ffi.Radiance(n_samples=n_samples, first_sample=first_sample, first_ray=first_ray, flags=flags)


def _rays6(origins, directions) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([np.asarray(origins, np.float32).reshape(-1, 3),
                                                np.asarray(directions, np.float32).reshape(-1, 3)], axis=1))


def radiance(scene, params: RenderParams, origins, directions, n_samples: int, first_sample: int = 0,
             first_ray: int = 0, sum=None):
    """What rayColor returns along each ray, averaged over n_samples samples (zrt_radiance; the
    definition: zrt.h "radiance queries").  params gives traversal, prng, seed, max_depth and
    sample_chunk.  sum (float32[n, 4]): the sums of samples [0, first_sample) the call adds onto
    (ZRT_RQ_ACCUMULATE); updated in place.  Returns (rgb float32[n, 3], info dict)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    rays = _rays6(origins, directions)
    n = rays.shape[0]
    rgb = np.zeros((n, 3), np.float32)
    rq = radiance_settings(n_samples, first_sample, first_ray, ZRT_RQ_ACCUMULATE if sum is not None else 0)
    if sum is not None and (sum.dtype != np.float32 or sum.shape != (n, 4) or not sum.flags.c_contiguous):
        raise ValueError("sum must be a C-contiguous float32[n, 4]")
    info = _ffi.RadianceInfo()
    p = params.abi()
    f = C.POINTER(C.c_float)
    check(lib().zrt_radiance(view, C.byref(p), C.byref(rq), rays.ctypes.data_as(f), n,
                             sum.ctypes.data_as(f) if sum is not None else None, rgb.ctypes.data_as(f),
                             C.byref(info)))
    return rgb, info.as_dict()


def debug_radiance_plan(params: RenderParams, rq: _ffi.Radiance, n: int, cu_count: int = 256,
                        partial_cap_bytes: int = 0) -> dict:
    """How zrt_ctx_radiance launches n rays with these params and settings on a device of
    cu_count CUs (zrt_debug_radiance_plan; no device): chunks, items, rounds, parked bytes,
    grid and resident lanes.  Raises ZrtError for what the call would refuse."""
    out = _ffi.RadiancePlan()
    p = params.abi()
    check(lib().zrt_debug_radiance_plan(C.byref(p), C.byref(rq), n, cu_count, partial_cap_bytes, C.byref(out)))
    return out.as_dict()


def rays_equirect(origin, width: int, height: int) -> np.ndarray:
    """Rays of an equirectangular panorama from a point (zrt_rays_equirect; host only):
    float32[height, width, 6] {origin, direction}, row 0 the bottom."""
    o = np.ascontiguousarray(np.asarray(origin, np.float32).reshape(3))
    out = np.zeros((max(height, 0), max(width, 0), 6), np.float32)
    f = C.POINTER(C.c_float)
    check(lib().zrt_rays_equirect(o.ctypes.data_as(f), width, height, out.ctypes.data_as(f)))
    return out


def lens_init(kind: int, look_from, look_at, vup, vfov: float, aspect: float, aperture: float = 0.0,
              focus_dist: float = 1.0, fisheye_fov: float = 180.0) -> _ffi.Lens:
    """The lens of `kind` (ZRT_LENS_*) at a pose (zrt_lens_init; host only): camera_init's
    plane scaled to the focal distance, the lens axes, the fisheye's field of view in degrees."""
    f3 = C.c_float * 3
    out = _ffi.Lens()
    check(lib().zrt_lens_init(kind, f3(*look_from), f3(*look_at), f3(*vup), vfov, aspect, aperture, focus_dist,
                              fisheye_fov, C.byref(out)))
    return out


def lens_from_camera(kind: int, camera: _ffi.Camera, aperture: float = 0.0, focus_dist: float = 0.0,
                     fisheye_fov: float = 180.0) -> _ffi.Lens:
    """The lens of `kind` at the pose of a camera (zrt_lens_from_camera; host only);
    focus_dist 0 keeps the camera's own plane."""
    out = _ffi.Lens()
    check(lib().zrt_lens_from_camera(kind, C.byref(camera), aperture, focus_dist, fisheye_fov, C.byref(out)))
    return out


def camera_query(x0: int, y0: int, w: int, h: int, n_samples: int, first_sample: int = 0,
                 flags: int = 0) -> _ffi.CameraQuery:
    """A zrt_camera_query: the pixel rectangle, n_samples samples per pixel from the pixel's
    sample first_sample; flags: ZRT_CQ_ACCUMULATE."""
    return _ffi.CameraQuery(x0=x0, y0=y0, w=w, h=h, n_samples=n_samples, first_sample=first_sample, flags=flags)


def render_lens(scene, params: RenderParams, lens: _ffi.Lens, n_samples: int, rect=None, first_sample: int = 0,
                sum=None, rgb=None):
    """A frame (or the rectangle rect = (x0, y0, w, h) of it) through a lens (zrt_render_lens;
    the definition: zrt.h "camera queries").  params gives width, height, traversal, prng, seed,
    max_depth and sample_chunk.  sum (float32[height, width, 4]): updated in place; with
    first_sample > 0 the call adds onto it (ZRT_CQ_ACCUMULATE).  rgb (float32[height, width, 3]):
    written inside the rectangle, kept outside it.  Returns (rgb, info dict)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    w, h = params.width, params.height
    x0, y0, rw, rh = rect if rect is not None else (0, 0, w, h)
    q = camera_query(x0, y0, rw, rh, n_samples, first_sample, ZRT_CQ_ACCUMULATE if first_sample else 0)
    if rgb is None:
        rgb = np.zeros((h, w, 3), np.float32)
    for a, c in ((sum, 4), (rgb, 3)):
        if a is not None and (a.dtype != np.float32 or a.shape != (h, w, c) or not a.flags.c_contiguous):
            raise ValueError(f"sum and rgb must be C-contiguous float32[height, width, {c}]")
    if first_sample and sum is None:
        raise ValueError("first_sample > 0 needs the sums of the samples before it")
    info = _ffi.RadianceInfo()
    p = params.abi()
    f = C.POINTER(C.c_float)
    check(lib().zrt_render_lens(view, C.byref(p), C.byref(lens), C.byref(q),
                                sum.ctypes.data_as(f) if sum is not None else None, rgb.ctypes.data_as(f),
                                C.byref(info)))
    return rgb, info.as_dict()


def debug_camera_plan(params: RenderParams, q: _ffi.CameraQuery, cu_count: int = 256,
                      partial_cap_bytes: int = 0) -> dict:
    """How zrt_ctx_camera launches this query (zrt_debug_camera_plan; no device): slots, tiles
    and the radiance plan over the slots.  Raises ZrtError for what the call would refuse."""
    out = _ffi.CameraPlan()
    p = params.abi()
    check(lib().zrt_debug_camera_plan(C.byref(p), C.byref(q), cu_count, partial_cap_bytes, C.byref(out)))
    return out.as_dict()


def lens_check(lens: _ffi.Lens) -> None:
    """Raises ZrtError for a lens zrt_ctx_camera would refuse (zrt_lens_check; no device)."""
    check(lib().zrt_lens_check(C.byref(lens)))


def rect(x0: int, y0: int, w: int, h: int) -> _ffi.Rect:
    """A zrt_rect: a pixel rectangle of the frame."""
    return _ffi.Rect(x0=x0, y0=y0, w=w, h=h)


def rect_check(params: RenderParams, r: _ffi.Rect) -> None:
    """Raises ZrtError for a rectangle (or a frame) the lens post calls would refuse
    (zrt_rect_check; no device)."""
    p = params.abi()
    check(lib().zrt_rect_check(C.byref(p), C.byref(r)))


def render_lens_denoised(scene, params: RenderParams, lens: _ffi.Lens, n_samples: int, rect=None,
                         denoise: _ffi.Denoise = None, guided: bool = True, flags: int = None):
    """A lens frame (or its rectangle rect = (x0, y0, w, h)) rendered and filtered
    (zrt_render_lens_denoised; the definition: zrt.h "denoising lens frames"): the camera query
    with moments, lens features, the variance plane and the guided filter over the rectangle;
    guided False: the plain a-trous filter.  denoise None: the matching defaults; flags None:
    the guided defaults' flags (0 for the plain filter).  Returns (rgb, dict) with noisy,
    features, variance (guided), info and denoise_ms in the dict."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    w, h = params.width, params.height
    x0, y0, rw, rh = rect if rect is not None else (0, 0, w, h)
    q = camera_query(x0, y0, rw, rh, n_samples)
    if flags is None:
        flags = denoise_guided_defaults()[1] if guided else 0
    rgb = np.zeros((h, w, 3), np.float32)
    noisy = np.zeros((h, w, 3), np.float32)
    features = np.zeros((h, w, 8), np.float32)
    variance = np.zeros((h, w), np.float32) if guided else None
    info = _ffi.RadianceInfo()
    ms = C.c_double()
    p = params.abi()
    f = C.POINTER(C.c_float)
    check(lib().zrt_render_lens_denoised(view, C.byref(p), C.byref(lens), C.byref(q),
                                         C.byref(denoise) if denoise is not None else None, 1 if guided else 0, flags,
                                         rgb.ctypes.data_as(f), noisy.ctypes.data_as(f), features.ctypes.data_as(f),
                                         variance.ctypes.data_as(f) if guided else None, C.byref(info), C.byref(ms)))
    return rgb, {"noisy": noisy, "features": features, "variance": variance, "info": info.as_dict(),
                 "denoise_ms": ms.value}


class RenderContext:
    """Device-resident scene (zrt_ctx_*): build + upload once, render many."""

    def __init__(self, scene, params: RenderParams):
        view = scene.view if isinstance(scene, LoadedScene) else scene
        self._scene = scene  # keep the host arrays alive while the ctx exists
        h = C.c_void_p()
        p = params.abi()
        check(lib().zrt_ctx_create(view, C.byref(p), C.byref(h)))
        self._h = h

    def tile_count(self, params: RenderParams) -> int:
        n = C.c_uint32()
        p = params.abi()
        check(lib().zrt_ctx_tile_count(self._h, C.byref(p), C.byref(n)))
        return n.value

    def render_tiles(self, camera, params: RenderParams, dev_tiles: int, stream: int = 0):
        p = params.abi()
        check(lib().zrt_ctx_render_tiles(self._h, C.byref(camera), C.byref(p),
                                         C.c_void_p(dev_tiles), C.c_void_p(stream or None)))

    def assemble(self, params: RenderParams, dev_gathered: int, dev_frame: int, stream: int = 0):
        p = params.abi()
        check(lib().zrt_ctx_assemble(self._h, C.byref(p), C.c_void_p(dev_gathered),
                                     C.c_void_p(dev_frame), C.c_void_p(stream or None)))

    def accum_begin(self, camera, params: RenderParams):
        """Start an accumulation run (zrt_ctx_accum_begin): params.samples_per_pixel is its cap."""
        p = params.abi()
        check(lib().zrt_ctx_accum_begin(self._h, C.byref(camera), C.byref(p)))

    def accum_pass(self, n_samples: int, dev_tiles: int, stream: int = 0):
        """Render the run's next n_samples samples per pixel, accumulate them and write the
        resolved tiles (zrt_ctx_accum_pass; asynchronous)."""
        check(lib().zrt_ctx_accum_pass(self._h, n_samples, C.c_void_p(dev_tiles), C.c_void_p(stream or None)))

    def accum_info(self) -> dict:
        """The last pass's metrics and times (zrt_ctx_accum_info; waits for it)."""
        out = _ffi.PassInfo()
        check(lib().zrt_ctx_accum_info(self._h, C.byref(out)))
        return out.as_dict()

    def adapt_begin(self, camera, params: RenderParams, tolerance: float, first_level: int = 0):
        """Start an adaptive run (zrt_ctx_adapt_begin): params.samples_per_pixel is its cap."""
        p = params.abi()
        ad = _adaptive(tolerance, first_level)
        check(lib().zrt_ctx_adapt_begin(self._h, C.byref(camera), C.byref(p), C.byref(ad)))
        self._adapt_tiles = self.tile_count(params)

    def adapt_level(self, dev_tiles: int, stream: int = 0) -> dict:
        """Render and resolve the run's next level over the tiles still active
        (zrt_ctx_adapt_level; returns once the surviving count is known): the level's info.
        dev_tiles must be the same buffer for the whole run."""
        out = _ffi.LevelInfo()
        check(lib().zrt_ctx_adapt_level(self._h, C.c_void_p(dev_tiles), C.c_void_p(stream or None), C.byref(out)))
        return out.as_dict()

    def adapt_samples(self) -> np.ndarray:
        """Samples per pixel of each local tile so far (zrt_ctx_adapt_samples)."""
        n = getattr(self, "_adapt_tiles", 0)
        out = np.zeros(max(1, n), dtype=np.uint32)
        check(lib().zrt_ctx_adapt_samples(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32)), n))
        return out[:n]

    def features(self, camera, params: RenderParams, dev_ptr: int, stream: int = 0):
        """The frame's first-hit feature buffer (zrt_ctx_features; asynchronous): width *
        height * 8 f32 at the device pointer dev_ptr - {N.xyz, t} and {A.rgb, id bits} per pixel."""
        p = params.abi()
        check(lib().zrt_ctx_features(self._h, C.byref(camera), C.byref(p), C.c_void_p(dev_ptr),
                                     C.c_void_p(stream or None)))

    def trace(self, params: RenderParams, dev_rays: int, n: int, dev_t: int, dev_prim: int, stream: int = 0):
        """Closest hit of n rays on the resident scene (zrt_ctx_trace; device pointers,
        asynchronous): rays n x {origin, direction} f32, t f32[n] (+inf on a miss), prim
        int32[n] (the index in the scene's list, -1 on a miss)."""
        p = params.abi()
        check(lib().zrt_ctx_trace(self._h, C.byref(p), C.c_void_p(dev_rays or None), n, C.c_void_p(dev_t or None),
                                  C.c_void_p(dev_prim or None), C.c_void_p(stream or None)))

    def occluded(self, params: RenderParams, dev_rays: int, dev_t_max: int, n: int, dev_out: int, stream: int = 0):
        """Any hit of n rays in (0.001, t_max) (zrt_ctx_occluded; device pointers, asynchronous):
        dev_t_max f32[n] or 0 = +inf for every ray; dev_out n bytes, 1 occluded / 0 not."""
        p = params.abi()
        check(lib().zrt_ctx_occluded(self._h, C.byref(p), C.c_void_p(dev_rays or None), C.c_void_p(dev_t_max or None),
                                     n, C.c_void_p(dev_out or None), C.c_void_p(stream or None)))

    def ao(self, camera, params: RenderParams, ao: _ffi.Ao, dev_features: int, dev_clear: int, dev_ao: int = 0,
           stream: int = 0):
        """Ambient occlusion from a feature buffer (zrt_ctx_ao; device pointers, asynchronous):
        dev_clear width * height u32 receives per pixel the AO rays that got away, dev_ao
        (0: not wanted) width * height f32 their share."""
        p = params.abi()
        check(lib().zrt_ctx_ao(self._h, C.byref(camera), C.byref(p), C.byref(ao), C.c_void_p(dev_features or None),
                               C.c_void_p(dev_clear or None), C.c_void_p(dev_ao or None), C.c_void_p(stream or None)))

    def radiance(self, params: RenderParams, rq: _ffi.Radiance, dev_rays: int, n: int, dev_sum: int,
                 dev_rgb: int = 0, stream: int = 0):
        """rayColor along n rays on the resident scene (zrt_ctx_radiance; device pointers,
        asynchronous): rays n x {origin, direction} f32; dev_sum n float4 {r, g, b, 0} receives
        the sample sums (read first under ZRT_RQ_ACCUMULATE), dev_rgb (0: not wanted) n x 3 f32
        their mean."""
        p = params.abi()
        check(lib().zrt_ctx_radiance(self._h, C.byref(p), C.byref(rq), C.c_void_p(dev_rays or None), n,
                                     C.c_void_p(dev_sum or None), C.c_void_p(dev_rgb or None),
                                     C.c_void_p(stream or None)))

    def camera(self, params: RenderParams, lens: _ffi.Lens, q: _ffi.CameraQuery, dev_sum: int, dev_rgb: int = 0,
               stream: int = 0):
        """A pixel rectangle of a frame through a lens on the resident scene (zrt_ctx_camera;
        device pointers, asynchronous): dev_sum width * height float4 and dev_rgb (0: not wanted)
        width * height * 3 f32 are whole-frame buffers; only the rectangle's pixels are written."""
        p = params.abi()
        check(lib().zrt_ctx_camera(self._h, C.byref(p), C.byref(lens), C.byref(q), C.c_void_p(dev_sum or None),
                                   C.c_void_p(dev_rgb or None), C.c_void_p(stream or None)))

    def camera_moments(self, params: RenderParams, lens: _ffi.Lens, q: _ffi.CameraQuery, dev_sum: int,
                       dev_rgb: int = 0, stream: int = 0):
        """camera() whose sums' fourth lane carries Q, the second moment of the chunk sums
        (zrt_ctx_camera_moments): what camera_variance() reads."""
        p = params.abi()
        check(lib().zrt_ctx_camera_moments(self._h, C.byref(p), C.byref(lens), C.byref(q),
                                           C.c_void_p(dev_sum or None), C.c_void_p(dev_rgb or None),
                                           C.c_void_p(stream or None)))

    def camera_features(self, params: RenderParams, lens: _ffi.Lens, r: _ffi.Rect, dev_features: int,
                        stream: int = 0):
        """The first-hit features of the rectangle's pixels along the lens' centre rays
        (zrt_ctx_camera_features; a query): features()' buffer, written inside the rectangle only."""
        p = params.abi()
        check(lib().zrt_ctx_camera_features(self._h, C.byref(p), C.byref(lens), C.byref(r),
                                            C.c_void_p(dev_features or None), C.c_void_p(stream or None)))

    def camera_variance(self, params: RenderParams, r: _ffi.Rect, n_total: int, dev_sum: int, dev_variance: int,
                        stream: int = 0):
        """The variance plane (width * height f32, the frame's layout) of camera_moments()' sums
        after n_total samples per pixel, over the rectangle (zrt_ctx_camera_variance)."""
        p = params.abi()
        check(lib().zrt_ctx_camera_variance(self._h, C.byref(p), C.byref(r), n_total, C.c_void_p(dev_sum or None),
                                            C.c_void_p(dev_variance or None), C.c_void_p(stream or None)))

    def denoise_rect(self, params: RenderParams, dn: _ffi.Denoise, flags: int, r: _ffi.Rect, dev_frame: int,
                     dev_features: int, dev_variance: int, dev_out: int, dev_out_variance: int = 0, stream: int = 0):
        """denoise() (dev_variance 0) or denoise_guided() with the rectangle as the filter's
        domain (zrt_ctx_denoise_rect): taps outside it are skipped, pixels outside it copied."""
        p = params.abi()
        check(lib().zrt_ctx_denoise_rect(self._h, C.byref(p), C.byref(dn), flags, C.byref(r),
                                         C.c_void_p(dev_frame or None), C.c_void_p(dev_features or None),
                                         C.c_void_p(dev_variance or None), C.c_void_p(dev_out or None),
                                         C.c_void_p(dev_out_variance or None), C.c_void_p(stream or None)))

    def camera_info(self) -> dict:
        """The last camera() call's counters and kernel time (zrt_ctx_camera_info; waits for it)."""
        out = _ffi.RadianceInfo()
        check(lib().zrt_ctx_camera_info(self._h, C.byref(out)))
        return out.as_dict()

    def radiance_info(self) -> dict:
        """The last radiance() call's counters and kernel time (zrt_ctx_radiance_info; waits for it)."""
        out = _ffi.RadianceInfo()
        check(lib().zrt_ctx_radiance_info(self._h, C.byref(out)))
        return out.as_dict()

    def debug_radiance(self) -> dict:
        """The last radiance() call's plan and deepest path (zrt_ctx_debug_radiance; waits for it)."""
        out = (C.c_uint32 * 4)()
        check(lib().zrt_ctx_debug_radiance(self._h, out))
        return dict(zip(("att_lds_rows", "deepest_path_rows", "stack_lds_rows", "grid"), out))

    def ao_ms(self) -> float:
        """Device time of the last ao() kernel in ms (zrt_ctx_ao_ms; waits for it)."""
        ms = C.c_double()
        check(lib().zrt_ctx_ao_ms(self._h, C.byref(ms)))
        return ms.value

    def query_ms(self) -> float:
        """Device time of the last trace() / occluded() kernel in ms (zrt_ctx_query_ms; waits for it)."""
        ms = C.c_double()
        check(lib().zrt_ctx_query_ms(self._h, C.byref(ms)))
        return ms.value

    def denoise(self, params: RenderParams, dn: _ffi.Denoise, dev_frame: int, dev_features: int, dev_out: int,
                stream: int = 0):
        """Filter the frame at dev_frame into dev_out, guided by the feature buffer at
        dev_features (zrt_ctx_denoise; device pointers, asynchronous; the definition: zrt.h)."""
        p = params.abi()
        check(lib().zrt_ctx_denoise(self._h, C.byref(p), C.byref(dn), C.c_void_p(dev_frame),
                                    C.c_void_p(dev_features), C.c_void_p(dev_out), C.c_void_p(stream or None)))

    def accum_variance(self, dev_tiles_var: int, stream: int = 0):
        """The live run's variance plane (zrt_ctx_accum_variance): one f32 per pixel of this
        rank's tiles, tile-major, at the device pointer dev_tiles_var."""
        check(lib().zrt_ctx_accum_variance(self._h, C.c_void_p(dev_tiles_var), C.c_void_p(stream or None)))

    def assemble_plane(self, params: RenderParams, dev_gathered: int, dev_frame: int, stride_tiles: int = 0,
                       stream: int = 0):
        """assemble() / assemble_padded() for one-channel planes (zrt_ctx_assemble_plane;
        stride_tiles 0: packed rank after rank)."""
        p = params.abi()
        check(lib().zrt_ctx_assemble_plane(self._h, C.byref(p), C.c_void_p(dev_gathered), stride_tiles,
                                           C.c_void_p(dev_frame), C.c_void_p(stream or None)))

    def denoise_guided(self, params: RenderParams, dn: _ffi.Denoise, flags: int, dev_frame: int, dev_features: int,
                       dev_variance: int, dev_out: int, dev_out_variance: int = 0, stream: int = 0):
        """denoise() with the variance-guided filter (zrt_ctx_denoise_guided): dev_variance is
        width * height f32 in the frame's layout, dev_out_variance (0: not wanted) receives the
        filtered variance."""
        p = params.abi()
        check(lib().zrt_ctx_denoise_guided(self._h, C.byref(p), C.byref(dn), flags, C.c_void_p(dev_frame),
                                           C.c_void_p(dev_features), C.c_void_p(dev_variance or None),
                                           C.c_void_p(dev_out), C.c_void_p(dev_out_variance or None),
                                           C.c_void_p(stream or None)))

    def temporal(self, camera, params: RenderParams, tp: _ffi.Temporal, dev_frame: int, dev_features: int,
                 dev_variance: int, dev_out: int, dev_out_variance: int = 0, dev_out_len: int = 0, stream: int = 0):
        """One frame of the temporal accumulation (zrt_ctx_temporal; device pointers,
        asynchronous; the definition: zrt.h): the context's history reprojected from the
        previous call's camera and blended into the frame at dev_frame."""
        p = params.abi()
        check(lib().zrt_ctx_temporal(self._h, C.byref(camera), C.byref(p), C.byref(tp), C.c_void_p(dev_frame or None),
                                     C.c_void_p(dev_features or None), C.c_void_p(dev_variance or None),
                                     C.c_void_p(dev_out or None), C.c_void_p(dev_out_variance or None),
                                     C.c_void_p(dev_out_len or None), C.c_void_p(stream or None)))

    def temporal_reset(self):
        """Drop the temporal history (zrt_ctx_temporal_reset)."""
        check(lib().zrt_ctx_temporal_reset(self._h))

    def temporal_ms(self) -> float:
        """Device time of the last temporal() in ms (zrt_ctx_temporal_ms; waits for it)."""
        ms = C.c_double()
        check(lib().zrt_ctx_temporal_ms(self._h, C.byref(ms)))
        return ms.value

    def denoise_ms(self) -> float:
        """Device time of the last denoise() in ms (zrt_ctx_denoise_ms; waits for it)."""
        ms = C.c_double()
        check(lib().zrt_ctx_denoise_ms(self._h, C.byref(ms)))
        return ms.value

    def sync(self):
        """Wait for the last launch; raises ZrtError on a device error (zrt_ctx_sync)."""
        check(lib().zrt_ctx_sync(self._h))

    def assemble_padded(self, params: RenderParams, dev_gathered: int, stride_tiles: int, dev_frame: int,
                        stream: int = 0):
        """Assemble from a gather of equal per-rank counts: rank r at tile r * stride_tiles."""
        p = params.abi()
        check(lib().zrt_ctx_assemble_padded(self._h, C.byref(p), C.c_void_p(dev_gathered), stride_tiles,
                                            C.c_void_p(dev_frame), C.c_void_p(stream or None)))

    def scanlines(self, height: int) -> np.ndarray:
        """This rank's per-scanline counters of the last launch (ZRT_FLAG_SCANLINES)."""
        rows = (_ffi.Scanline * height)()
        check(lib().zrt_ctx_scanlines(self._h, rows, height))
        return _scanlines_np(rows)

    def stats(self) -> dict:
        st = _ffi.Stats()
        check(lib().zrt_ctx_stats(self._h, C.byref(st)))
        return st.as_dict()

    def debug_counters(self, n: int = 48):
        out = (C.c_uint64 * n)()
        check(lib().zrt_ctx_debug_counters(self._h, out, n))
        return list(out)

    def debug_wave_times(self, cap: int = 1 << 16):
        """ZRT_PROFILE builds: array[n_waves, 2] of (start, end) 100 MHz stamps of the last launch."""
        out = np.zeros(cap, np.uint64)
        n = C.c_uint32()
        check(lib().zrt_ctx_debug_wave_times(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), cap, C.byref(n)))
        return out[: 2 * n.value].reshape(-1, 2).copy()

    def debug_schedule(self, cap: int = 1 << 20):
        """(probe cost per local tile, tile order) of the last launch; empty if unscheduled."""
        costs = np.zeros(cap, np.uint32)
        order = np.zeros(cap, np.uint32)
        n = C.c_uint32()
        check(lib().zrt_ctx_debug_schedule(self._h, costs.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           order.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n)))
        return costs[: n.value].copy(), order[: n.value].copy()

    def kernel_ms(self) -> float:
        ms = C.c_double()
        check(lib().zrt_ctx_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def close(self):
        if getattr(self, "_h", None):
            lib().zrt_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def bvh_build(scene):
    """The product's BVH (zrt_bvh_build) as numpy arrays (mins, maxs, left, right, max_depth)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    nodes = C.POINTER(_ffi.BvhNode)()
    n = C.c_uint32()
    depth = C.c_uint32()
    check(lib().zrt_bvh_build(view, C.byref(nodes), C.byref(n), C.byref(depth)))
    try:
        return nodes_to_numpy(nodes, n.value) + (depth.value,)
    finally:
        lib().zrt_free(C.cast(nodes, C.c_void_p))


def bvh_build_device(scene, device: int = 0):
    """The same BVH built on the GPU (zrt_bvh_build_device), as bvh_build returns it."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    nodes = C.POINTER(_ffi.BvhNode)()
    n = C.c_uint32()
    depth = C.c_uint32()
    check(lib().zrt_bvh_build_device(view, device, C.byref(nodes), C.byref(n), C.byref(depth)))
    try:
        return nodes_to_numpy(nodes, n.value) + (depth.value,)
    finally:
        lib().zrt_free(C.cast(nodes, C.c_void_p))


def nodes_to_numpy(nodes, n):
    dt = np.dtype([("min", "<f4", 3), ("left", "<i4"), ("max", "<f4", 3), ("right", "<i4")])
    buf = np.ctypeslib.as_array(C.cast(nodes, C.POINTER(C.c_uint8)), shape=(n * 32,)).copy()
    a = buf.view(dt)
    return a["min"].copy(), a["max"].copy(), a["left"].copy(), a["right"].copy()


def debug_division(n: int = 1 << 30, device: int = 0) -> dict:
    """Device self-check of the kernel's short correctly rounded divisions
    (zrt_debug_division): mismatch counts against HIP's IEEE `/`."""
    out = (C.c_uint64 * 5)()
    check(lib().zrt_debug_division(n, out, device))
    return dict(zip(("rcp_sqrt_all_2p32", "div", "unit", "inv_dir", "jitter"), (int(v) for v in out)))


def debug_math(fn: int, x, y=None, device: int = 0):
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty_like(x)
    yp = None
    if y is not None:
        y = np.ascontiguousarray(y, dtype=np.float32)
        yp = y.ctypes.data_as(C.POINTER(C.c_float))
    check(lib().zrt_debug_math(fn, x.ctypes.data_as(C.POINTER(C.c_float)), yp,
                               out.ctypes.data_as(C.POINTER(C.c_float)), x.size, device))
    return out


def debug_rng(prng: int, key: int, n: int, device: int = 0):
    out = np.empty(n, dtype=np.uint64)
    check(lib().zrt_debug_rng(prng, key, out.ctypes.data_as(C.POINTER(C.c_uint64)), n, device))
    return out


def debug_compact(list_, tile_done, fill: int = 0xFFFFFFFF, device: int = 0):
    """One launch of the adaptive run's compaction (zrt_debug_compact) over list_ (entries
    index tile_done; bit 31 of a tile_done word = frozen).  The output buffer starts as
    len(list_) words of `fill`.  Returns (out, count): the whole buffer after the launch
    and the number of entries the kernel reports written."""
    u32p = C.POINTER(C.c_uint32)
    lst = np.ascontiguousarray(list_, dtype=np.uint32)
    done = np.ascontiguousarray(tile_done, dtype=np.uint32)
    out = np.full(lst.size, fill, dtype=np.uint32)
    count = C.c_uint32()
    check(lib().zrt_debug_compact(lst.ctypes.data_as(u32p), lst.size, done.ctypes.data_as(u32p), done.size,
                                  out.ctypes.data_as(u32p), C.byref(count), device))
    return out, count.value


def read_png(path: str):
    """png_image.readFile (zrt_image_read_png): float32[height, width, 3], row 0 = bottom, c/255."""
    w, h, px = C.c_uint32(), C.c_uint32(), C.POINTER(C.c_float)()
    check(lib().zrt_image_read_png(path.encode(), C.byref(w), C.byref(h), C.byref(px)))
    try:
        return np.ctypeslib.as_array(px, shape=(h.value, w.value, 3)).copy()
    finally:
        lib().zrt_free(px)


def write_png(path: str, image) -> None:
    """png_image.writeFile (png_image.zig:96-148) for a framebuffer[H, W, 3] (row 0 = bottom)."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w, _ = img.shape
    check(lib().zrt_image_write_png(os.fsencode(path), img.ctypes.data_as(C.POINTER(C.c_float)), w, h))


def write_ppm(path: str, image) -> None:
    """ppm_image.writeFile (plain P3) for a framebuffer[H, W, 3] (row 0 = bottom)."""
    img = np.ascontiguousarray(image, dtype=np.float32)
    h, w, _ = img.shape
    check(lib().zrt_image_write_ppm(os.fsencode(path), img.ctypes.data_as(C.POINTER(C.c_float)), w, h))


def debug_lds_plans(scene) -> int:
    """Host-side check of every LDS layout the launch code can plan for this scene
    (zrt_debug_lds_plans; no device): returns the number of plans checked, raises
    ZrtError naming the first overlapping / misaligned / oversized region."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    n = C.c_uint32()
    check(lib().zrt_debug_lds_plans(view, C.byref(n)))
    return n.value


def debug_buffer_plans(scene, legacy: bool = False) -> int:
    """Host-side check of the global attenuation / stack-overflow rows a FAST frame's
    launches share (zrt_debug_buffer_plans; no device): zrt_render's sizing against
    the need of the render launch and of its scheduling probe, for every loop, stack
    width, PRNG, node format and a range of depths and grids.  Returns the number of
    configurations checked, raises ZrtError naming the first launch whose rows would
    lie past its buffer.  legacy=True applies the sizing before the round-5 fix."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    n = C.c_uint32()
    check(lib().zrt_debug_buffer_plans(view, 1 if legacy else 0, C.byref(n)))
    return n.value


def debug_launch_plan(scene, params) -> dict:
    """The launch decision a render of this scene with these params would take
    (zrt_debug_launch_plan; no device), under the environment knobs a real launch
    reads: the zrt_launch_plan fields as a dict (kmode, stk16, stack_rows,
    stack_depth, att_rows, att_rows_per_path, mats_in_lds, ...)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = _ffi.LaunchPlan()
    p = params.abi()
    check(lib().zrt_debug_launch_plan(view, C.byref(p), C.byref(out)))
    return out.as_dict()


def debug_lean_kernel(scene, camera, params) -> bool:
    """Whether a render of this scene from this camera with these params would launch
    the lean lockstep kernel (zrt_debug_lean_kernel; no device), under the
    environment knobs a real launch reads (ZRT_LEAN among them)."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    out = C.c_uint32()
    p = params.abi()
    check(lib().zrt_debug_lean_kernel(view, C.byref(camera), C.byref(p), C.byref(out)))
    return bool(out.value)


ZRT_TILE_SKY = 0x80000000
ZRT_TILE_ONE_SPHERE = 0x40000000  # | the sphere's device primitive slot


def debug_tile_classes(scene, camera, params, one_sphere=False):
    """The class word of each of this rank's 8x8 tiles as a render of this scene from
    this camera with these params would split them (zrt_debug_tile_classes; no device),
    under the environment knobs a real launch reads (ZRT_SKY_TILES among them): a
    uint32 array (0 general, ZRT_TILE_SKY all sky, ZRT_TILE_ONE_SPHERE | slot for a tile
    whose primary rays can hit that one sphere alone) and a dict of the classifier's
    margins (sphere_reach, tri_reach, k_ao, k_c).  one_sphere=False (the default, what
    callers that know the sky class alone expect) reports a one-sphere tile as general."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    p = params.abi()
    n, n_sky = C.c_uint32(), C.c_uint32()
    m = (C.c_double * 4)()
    check(lib().zrt_debug_tile_classes(view, C.byref(camera), C.byref(p), None, 0, C.byref(n), C.byref(n_sky), m))
    out = np.zeros(max(1, n.value), dtype=np.uint32)
    check(lib().zrt_debug_tile_classes(view, C.byref(camera), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       n.value, C.byref(n), C.byref(n_sky), m))
    out = out[:n.value]
    assert int((out == ZRT_TILE_SKY).sum()) == n_sky.value
    if not one_sphere:
        out[(out & ZRT_TILE_SKY) == 0] = 0
    return out, dict(sphere_reach=m[0], tri_reach=m[1], k_ao=m[2], k_c=m[3])


def debug_slot_prims(scene, params):
    """The list index of the primitive in each device primitive slot (zrt_debug_slot_prims; no
    device): a uint32 array indexed by slot, e.g. by the slot bits of a one-sphere class word."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    p = params.abi()
    n = C.c_uint32()
    check(lib().zrt_debug_slot_prims(view, C.byref(p), None, 0, C.byref(n)))
    out = np.zeros(max(1, n.value), dtype=np.uint32)
    check(lib().zrt_debug_slot_prims(view, C.byref(p), out.ctypes.data_as(C.POINTER(C.c_uint32)), n.value, C.byref(n)))
    return out[:n.value]


def debug_qnodes(scene) -> int:
    """Host-side check of the scene's compressed wide nodes (zrt_debug_qnodes; no
    device): returns the number of slots checked, raises ZrtError on a violation."""
    view = scene.view if isinstance(scene, LoadedScene) else scene
    n = C.c_uint64()
    check(lib().zrt_debug_qnodes(view, C.byref(n)))
    return n.value


def debug_octant_offsets(stride_f4: int, n_top: int, node_f4: int = 8) -> None:
    """The size check context creation makes on a flattened wide tree
    (zrt_debug_octant_offsets; no device): raises ZrtError(ZRT_E_UNSUPPORTED) for a
    tree whose octant stride or LDS top levels reach 2^24 float4s."""
    check(lib().zrt_debug_octant_offsets(stride_f4, n_top, node_f4))
