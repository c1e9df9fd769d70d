"""A scene with one material per sphere: a material table of any size.

The lockstep and list-lane loops read the material table from LDS only
(render.hip render_loop / render_loop_list); n_side chooses whether the table fits their
share of the block's LDS (48 B per material on the device, ~26 KiB share) or
the launch has to fall back to a loop that reads it from global memory.
"""
import ctypes as C

import numpy as np

import zraytrace_amd as z
from zraytrace_amd import _ffi


def many_materials_scene(n_side=24):
    """A grid of n_side^2 small spheres over a ground sphere, every one with a material
    of its own (lambertian / metal / dielectric in turn, each with a color texture):
    n_side^2 + 1 materials, 48 B each on the device - past the lockstep and list-lane
    loops' LDS share (~26 KiB per block) at n_side = 24."""
    n = n_side * n_side + 1
    rng = np.random.default_rng(5)
    cols = rng.random((n, 3), dtype=np.float32)
    texs = (_ffi.Texture * n)(*[_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(*map(float, cols[i])), 0.0, 0.0)
                                for i in range(n)])
    kinds = (_ffi.ZRT_MAT_LAMBERTIAN, _ffi.ZRT_MAT_METAL, _ffi.ZRT_MAT_DIELECTRIC)
    mats = (_ffi.Material * n)(*[_ffi.Material(kinds[i % 3], i, 0.3 if kinds[i % 3] == _ffi.ZRT_MAT_METAL
                                               else 1.5 if kinds[i % 3] == _ffi.ZRT_MAT_DIELECTRIC else 0.0)
                                 for i in range(n)])
    prims = (_ffi.Prim * n)()
    for i in range(n - 1):
        gx, gy = i % n_side, i // n_side
        prims[i].kind = _ffi.ZRT_PRIM_SPHERE
        prims[i].material = i
        prims[i].center = _ffi.Vec3(-2.3 + 0.2 * gx, -0.35, 2.0 + 0.2 * gy)
        prims[i].radius = 0.08
    prims[n - 1].kind = _ffi.ZRT_PRIM_SPHERE
    prims[n - 1].material = n - 1
    prims[n - 1].center = _ffi.Vec3(0.0, -100.5, 3.0)
    prims[n - 1].radius = 100.0
    scene = _ffi.Scene(prims, n, n, mats, texs, n, 0, C.cast(None, C.POINTER(_ffi.Image)))
    scene._keep = (prims, mats, texs)
    return scene


def camera(n_side=24):
    """n_side = 24: the camera test_material_table_past_lds_share looks at the whole grid
    with; a smaller grid: a camera close above its centre, so that the frame is full of
    glass, metal and lambertian spheres and paths run deep."""
    if n_side == 24:
        return z.camera_init((0, 0.6, -1.0), (0, -0.3, 3.0), (0, 1, 0), 50.0, 1.0)
    cx, cz = -2.3 + 0.1 * (n_side - 1), 2.0 + 0.1 * (n_side - 1)
    return z.camera_init((cx, 0.1, cz - 1.0), (cx, -0.35, cz), (0, 1, 0), 50.0, 1.0)


# A grid whose 37 materials (1776 B) fit the lockstep loop's LDS share beside three
# attenuation rows (tests/test_host.py test_launch_plan_material_table_fallback)
N_SIDE_LOCKSTEP = 6
