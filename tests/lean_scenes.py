"""Four tiny BVH scenes around the lean lockstep kernel's conditions.

The lean kernel (render.hip struct Lean) is launched only for a scene of
solid-colour Lambertian and metal materials, rendered from inside the scene's
ray-origin bound.  Each scene here is a dozen triangles (a faceted mound) over a
ground sphere, built through ctypes as tests/many_materials.py builds its grid:

  "a"  solid Lambertian + solid metal: eligible
  "b"  = a plus one dielectric sphere
  "c"  = a with one image-textured material
  "d"  = a rendered from a camera outside the origin bound
"""
import ctypes as C
import math

import numpy as np

import zraytrace_amd as z
from zraytrace_amd import _ffi

NAMES = ("a", "b", "c", "d")
GROUND_R = 10.0


def _mound():
    """12 triangles: a six-sided pyramid and the six outward flaps at its foot."""
    tris = []
    apex = (0.0, 0.55, 0.0)
    ring = [(0.6 * math.cos(k * math.pi / 3.0), -0.3, 0.6 * math.sin(k * math.pi / 3.0)) for k in range(6)]
    outer = [(1.1 * math.cos((k + 0.5) * math.pi / 3.0), -0.45, 1.1 * math.sin((k + 0.5) * math.pi / 3.0))
             for k in range(6)]
    for k in range(6):
        a, b = ring[k], ring[(k + 1) % 6]
        tris.append((apex, b, a))      # (counter-clockwise seen from outside)
        tris.append((a, b, outer[k]))
    return tris


def scene(name):
    """The zrt_scene of one of NAMES (keep the returned object alive)."""
    assert name in NAMES
    tris = _mound()
    colors = [(0.2, 0.7, 0.25), (0.8, 0.8, 0.85), (0.7, 0.3, 0.2), (0.9, 0.9, 0.2)]
    n_tex = len(colors)
    texs = (_ffi.Texture * n_tex)(*[_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(*c), 0.0, 0.0) for c in colors])
    # ground: Lambertian green; the mound: metal, Lambertian red, metal yellow in turn
    mat_list = [_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0), _ffi.Material(_ffi.ZRT_MAT_METAL, 1, 0.0),
                _ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 2, 0.0), _ffi.Material(_ffi.ZRT_MAT_METAL, 3, 0.0)]
    images, keep = C.cast(None, C.POINTER(_ffi.Image)), []
    n_images = 0
    if name == "b":
        mat_list.append(_ffi.Material(_ffi.ZRT_MAT_DIELECTRIC, 0, 1.5))
    if name == "c":  # the red Lambertian facets take a 5 x 3 image instead (values k / 255 and others)
        px = np.random.default_rng(11).random((3, 5, 3), dtype=np.float32)
        px[0] = np.round(px[0] * 255.0).astype(np.float32) / np.float32(255.0)
        keep.append(px)
        imgs = (_ffi.Image * 1)(_ffi.Image(5, 3, px.ctypes.data_as(C.POINTER(C.c_float))))
        keep.append(imgs)
        images, n_images = C.cast(imgs, C.POINTER(_ffi.Image)), 1
        texs[2] = _ffi.Texture(_ffi.ZRT_TEX_IMAGE, 0, _ffi.Vec3(0.0, 0.0, 0.0), 0.25, 0.1)
    mats = (_ffi.Material * len(mat_list))(*mat_list)
    n = len(tris) + 1 + (1 if name == "b" else 0)
    prims = (_ffi.Prim * n)()
    for i, (a, b, c) in enumerate(tris):
        prims[i].kind = _ffi.ZRT_PRIM_TRIANGLE
        prims[i].material = 1 + i % 3
        prims[i].a, prims[i].b, prims[i].c = _ffi.Vec3(*a), _ffi.Vec3(*b), _ffi.Vec3(*c)
    g = len(tris)
    prims[g].kind = _ffi.ZRT_PRIM_SPHERE
    prims[g].material = 0
    prims[g].center = _ffi.Vec3(0.0, -0.5 - GROUND_R, 0.0)
    prims[g].radius = GROUND_R
    if name == "b":
        prims[g + 1].kind = _ffi.ZRT_PRIM_SPHERE
        prims[g + 1].material = len(mat_list) - 1
        prims[g + 1].center = _ffi.Vec3(0.9, -0.1, -0.9)
        prims[g + 1].radius = 0.4
    s = _ffi.Scene(prims, n, len(mat_list), mats, texs, n_tex, n_images, images)
    s._keep = (prims, mats, texs, keep)
    return s


def camera(name):
    """a-c: close to the mound.  d: far above it with a narrow lens - outside the bound
    (2 x the root box's largest half extent, about 2 x GROUND_R, from its centre)."""
    if name == "d":
        return z.camera_init((0.4, 45.0, -0.3), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 3.5, 1.0)
    return z.camera_init((1.6, 0.9, -2.2), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 1.0)


_CACHE = {}


def get(name):
    """(scene object, zrt_scene pointer, camera), built once per name."""
    if name not in _CACHE:
        s = scene(name)
        _CACHE[name] = (s, C.pointer(s), camera(name))
    return _CACHE[name]
