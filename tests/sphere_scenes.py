"""Synthetic scenes around the one-sphere tile class (tile_class.cpp; DESIGN.md §3
"One-sphere tiles"), shared by tests/test_one_sphere_classes.py and
tests/test_gpu_sphere_tiles.py.

Every scene has more than 10 primitives, so the reference builds a tree: one or two
large spheres and a cluster of twelve tiny triangles (tiny, so that their reach at the
reference's det floor stays small and tiles can be proved to miss them; in view, or
behind the camera where they only widen the tree's root box, and with it the ray-origin
bound, so that the camera lies inside it).

  "horizon"   a ground sphere under a horizontal camera, the cluster far off in view:
              the horizon crosses the frame, its tiles see the sphere's silhouette
  "overlap"   two spheres that overlap on screen
  "behind"    the horizon scene with a second sphere behind the camera
  "inside"    the camera inside a large sphere
  "two"       two disjoint spheres, the left one covering more tiles
  "all"       the camera looks down at a ground sphere that fills the frame
  "down_z"    the horizon scene seen down -z (an odd width puts u = 0.5 into the
              centre column's footprint; a random jitter almost never lands on it, so this
              scene alone does not produce a degenerate ray - "slit" does)
  "slit"      the horizon scene through a camera whose horizontal vector is 2^-110 long:
              every ray has |d.x| < 2^-100, i.e. is degenerate for the FAST traversal
"""
import ctypes as C

import numpy as np

import zraytrace_amd as z
from zraytrace_amd import _ffi

NAMES = ("horizon", "overlap", "behind", "inside", "two", "all", "down_z", "slit")


def cluster(centre, size=0.02, n=12):
    """n tiny triangles around `centre`, facing +z (towards the cameras used here)."""
    rng = np.random.default_rng(3)
    tris = []
    for _ in range(n):
        a = np.asarray(centre, np.float64) + rng.uniform(-0.3, 0.3, 3)
        tris.append(("t", a, a + (size, 0.0, 0.0), a + (0.0, size, 0.0)))
    return tris


def build(prims, extra=None):
    """A zrt_scene: spheres Lambertian grey, triangles metal.  extra: "dielectric" or
    "image" adds such a material to the table (no primitive uses it)."""
    texs = [_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.5, 0.6, 0.5), 0.0, 0.0),
            _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.8, 0.7, 0.6), 0.0, 0.0)]
    mats = [_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0), _ffi.Material(_ffi.ZRT_MAT_METAL, 1, 0.0)]
    images, n_images, keep = C.cast(None, C.POINTER(_ffi.Image)), 0, []
    if extra == "dielectric":
        mats.append(_ffi.Material(_ffi.ZRT_MAT_DIELECTRIC, 0, 1.5))
    elif extra == "image":
        px = np.full((2, 2, 3), 0.5, np.float32)
        imgs = (_ffi.Image * 1)(_ffi.Image(2, 2, px.ctypes.data_as(C.POINTER(C.c_float))))
        keep += [px, imgs]
        images, n_images = C.cast(imgs, C.POINTER(_ffi.Image)), 1
        texs.append(_ffi.Texture(_ffi.ZRT_TEX_IMAGE, 0, _ffi.Vec3(0.0, 0.0, 0.0), 0.0, 0.0))
        mats.append(_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 2, 0.0))
    else:
        assert extra is None
    tarr = (_ffi.Texture * len(texs))(*texs)
    marr = (_ffi.Material * len(mats))(*mats)
    arr = (_ffi.Prim * len(prims))()
    for i, q in enumerate(prims):
        if q[0] == "s":
            arr[i].kind = _ffi.ZRT_PRIM_SPHERE
            arr[i].material = 0
            arr[i].center = _ffi.Vec3(*[float(x) for x in q[1]])
            arr[i].radius = float(q[2])
        else:
            arr[i].kind = _ffi.ZRT_PRIM_TRIANGLE
            arr[i].material = 1
            arr[i].a, arr[i].b, arr[i].c = (_ffi.Vec3(*[float(x) for x in v]) for v in q[1:4])
    s = _ffi.Scene(arr, len(prims), len(mats), marr, tarr, len(texs), n_images, images)
    s._keep = (arr, marr, tarr, keep)
    return s


GROUND = ("s", (0.0, -100.0, 0.0), 100.0)


def prims_of(name):
    if name in ("horizon", "down_z", "slit"):
        return [GROUND] + cluster((3.0, 2.5, -12.0))
    if name == "overlap":
        return [("s", (-0.6, 0.0, -6.0), 1.0), ("s", (0.6, 0.0, -8.0), 1.0)] + cluster((0.0, 2.0, 10.0))
    if name == "behind":
        return [GROUND, ("s", (0.0, 1.0, 8.0), 2.0)] + cluster((3.0, 2.5, -12.0))
    if name == "inside":
        return [("s", (0.0, 0.0, 0.0), 30.0)] + cluster((2.0, 1.0, -8.0))
    if name == "two":
        return [("s", (-2.0, 0.0, -8.0), 1.6), ("s", (2.6, 0.0, -8.0), 0.8)] + cluster((0.0, 2.0, 10.0))
    if name == "all":
        return [GROUND] + cluster((40.0, 1.0, 0.0))
    raise KeyError(name)


def camera_of(name):
    if name == "all":
        return z.camera_init((0.0, 3.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 40.0, 1.0)
    if name == "slit":
        cam = z.camera_init((0.0, 1.0, 0.0), (0.0, 1.0, -1.0), (0.0, 1.0, 0.0), 60.0, 1.0)
        cam.horizontal = _ffi.Vec3(2.0 ** -110, 0.0, 0.0)
        cam.lower_left_corner = _ffi.Vec3(0.0, cam.lower_left_corner.y, cam.lower_left_corner.z)
        return cam
    if name in ("horizon", "behind", "down_z"):
        return z.camera_init((0.0, 1.0, 0.0), (0.0, 1.0, -1.0), (0.0, 1.0, 0.0), 60.0, 1.0)
    return z.camera_init((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 50.0, 1.0)


_CACHE = {}


def get(name, extra=None):
    """(scene object, zrt_scene pointer, camera), built once."""
    k = (name, extra)
    if k not in _CACHE:
        s = build(prims_of(name), extra)
        _CACHE[k] = (s, C.pointer(s), camera_of(name))
    return _CACHE[k]


def sphere_indices(view):
    """List indices of the scene's spheres, largest radius first."""
    s = view.contents
    idx = [i for i in range(s.n_prims) if s.prims[i].kind == _ffi.ZRT_PRIM_SPHERE]
    return sorted(idx, key=lambda i: -s.prims[i].radius)
