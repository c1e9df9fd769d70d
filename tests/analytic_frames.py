"""Frames with a closed form: the geometry that says which pixels of a 16 x 16 frame lie wholly
on the floor or wholly on the sky, and what they must hold, in float64.

Test infrastructure beside tests/analytic_ref.py (whose floor, scene builder and Lambertian
moments it uses): tests/test_analytic_ref.py (CPU) and tests/test_gpu_analytic.py (GPU).

  a pixel wholly on the unoccluded floor   rho sky((2/3) n_y), whatever the camera or lens;
  a pinhole pixel wholly on the sky        the quadrature of sky(unit(getRay(u, v)).y) over
                                           u = (x + r1 - 0.5) / w, v = (y + r2 - 0.5) / h,
                                           r in [0, 1) (camera.zig:46-51, raytrace.zig:173-174);
  ambient occlusion under (e)'s sphere     1 - (r / d)^2 cos(beta) at the centre ray's hit point.
"""
import ctypes as C
import functools
import math

import numpy as np

from analytic_ref import (FLOOR, PAD_MAT, RHO, T_MIN, build_scene, f32, occlusion_form, padding, sky, sphere_t,
                          tilted_floor, tri_normal, unit)

FRAME_W = FRAME_H = 16
FRAME_POSE = ((0.0, 1.0, 6.0), (0.0, 1.35, 0.0), (0.0, 1.0, 0.0), 40.0, 1.0)  # Camera.init's arguments
DOWN_POSE = ((0.0, 4.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.0)  # every pixel on the floor
SPHERE_POSE = ((0.0, 0.5, 1.8), (0.0, 1.8, 0.0), (0.0, 1.0, 0.0), 50.0, 1.0)  # the unit sphere low in the frame
AO_POSE = ((2.5, 2.0, 3.0), (0.2, 0.0, 0.2), (0.0, 1.0, 0.0), 40.0, 1.0)  # the floor under and beside (e)'s sphere
HORIZON_ROWS = (6, 7)  # the rows the horizon (and, with it, the floor's far edges) crosses: left out
FLOOR_ROWS, SKY_ROWS = tuple(range(0, 6)), tuple(range(8, 16))


@functools.lru_cache(maxsize=None)
def floor_scene(bvh=False, tilt=0.0):
    """The floor alone, Lambertian RHO (a surface list of one primitive); bvh: padded with tiny
    spheres just under its middle, where every ray that goes down meets the floor first."""
    tri = tilted_floor(tilt) if tilt else FLOOR
    s = build_scene(padding((0.0, -0.6, 0.0), 0.3, 0.02, 1) if bvh else [], [tri + (0,)],
                    [("L", RHO)] + ([PAD_MAT] if bvh else []))
    return s, C.pointer(s)


def vec(v):
    return np.array([v.x, v.y, v.z], np.float64)


def lens_rays(lens, u, v, kind, disc=(0.0, 0.0)):
    """(origins, unit directions) of zrt.h's lens models at plane coordinates u, v (arrays), in
    float64: pinhole = Camera.getRay (camera.zig:46-51); thin: the origin moved by disc on the
    lens axes; ortho: from the plane point along axis_w; equirect and fisheye: by angle."""
    import zraytrace_amd as z
    u, v = np.asarray(u, np.float64)[..., None], np.asarray(v, np.float64)[..., None]
    org, plane = vec(lens.origin), vec(lens.lower_left_corner) + vec(lens.horizontal) * u + vec(lens.vertical) * v
    if kind != z.ZRT_LENS_PINHOLE:  # (a pinhole may be a plain zrt_camera, which has no axes)
        au, av, aw = vec(lens.axis_u), vec(lens.axis_v), vec(lens.axis_w)
    if kind in (z.ZRT_LENS_PINHOLE, z.ZRT_LENS_THIN):
        o = org + (au * disc[0] + av * disc[1] if kind == z.ZRT_LENS_THIN else 0.0) + 0 * plane
        d = plane - o
    elif kind == z.ZRT_LENS_ORTHO:
        o, d = plane, aw + 0 * plane
    elif kind == z.ZRT_LENS_EQUIRECT:
        phi, th = 2 * math.pi * u, math.pi * v
        o, d = org + 0 * plane, np.concatenate([np.sin(th) * np.cos(phi), -np.cos(th), np.sin(th) * np.sin(phi)], -1)
    else:
        px, py = 2 * u - 1, 2 * v - 1
        r = np.sqrt(px * px + py * py)
        th = r * float(lens.half_fov)
        k = np.where(r > 0, np.sin(th) / np.where(r > 0, r, 1.0), 0.0)
        o, d = org + 0 * plane, au * (px * k) + av * (py * k) + aw * np.cos(th)
    return o, d / np.sqrt((d * d).sum(-1, keepdims=True))


def footprint(x, y, w, h, lo=-0.5, k=9):
    """(u, v) grids over pixel (x, y)'s jitter range: u = (x + r1 - 0.5) / w, v = (y + r2 - 0.5)
    / h with r in [0, 1) (raytrace.zig:173-174); lo = 0 is the wrong model "jitter-0-1"."""
    r = np.linspace(0.0, 1.0, k)
    return np.meshgrid((x + r + lo) / w, (y + r + lo) / h, indexing="xy")


def on_floor(o, d, tri=FLOOR):
    """Where rays meet a floor triangle from its front (triangle.zig:55-63), 1 % inside its edges."""
    a, e1, e2 = f32(tri[0]), f32(tri[1]) - f32(tri[0]), f32(tri[2]) - f32(tri[0])
    fn = np.cross(e1, e2)
    det = -(d @ fn)
    with np.errstate(all="ignore"):
        ao = o - a
        dao = np.cross(ao, d)
        uu, vv, t = (dao @ e2) / det, -(dao @ e1) / det, (ao @ fn) / det
    return (det > 1e-4 * math.sqrt(fn @ fn)) & (t > T_MIN) & (uu > 0.01) & (vv > 0.01) & (uu + vv < 0.99)


def classify_pixels(lens, kind, w=FRAME_W, h=FRAME_H, tri=FLOOR):
    """int[h, w]: 1 where a pixel's whole jitter footprint (and, for the thin lens, the whole
    lens disc) meets the floor, 2 where all of it goes up to the sky, 0 otherwise."""
    discs = [(0.0, 0.0)] + [(math.cos(k * math.pi / 4), math.sin(k * math.pi / 4)) for k in range(8)]
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            rays = [lens_rays(lens, *footprint(x, y, w, h), kind, dc) for dc in discs]
            hit, up = (np.stack(a) for a in zip(*[(on_floor(o, d, tri), d[..., 1] > 0.02) for o, d in rays]))
            out[y, x] = 1 if hit.all() else 2 if up.all() else 0
    return out


def sky_pixels_beside_sphere(cam, centre, radius, w=FRAME_W, h=FRAME_H):
    """int[h, w]: 2 where every ray of a pinhole pixel's footprint passes the sphere at more than
    1.05 radius, 0 otherwise: the sky pixels of a frame that looks at a sphere alone."""
    out = np.zeros((h, w), np.int64)
    for y in range(h):
        for x in range(w):
            o, d = lens_rays(cam, *footprint(x, y, w, h), 0)
            oc = np.asarray(centre, np.float64) - o
            along = (oc * d).sum(-1)
            out[y, x] = 2 if ((oc * oc).sum(-1) - along * along > (1.05 * radius) ** 2).all() else 0
    return out


def sky_pixel(lens, x, y, w=FRAME_W, h=FRAME_H, model=None, k=64):
    """(mean, variance) of a pinhole pixel wholly on the sky: sky(unit(getRay(u, v)).y) over the
    jitter footprint, by a k x k midpoint rule in float64."""
    import zraytrace_amd as z
    r = (np.arange(k) + 0.5) / k
    lo = 0.0 if model == "jitter-0-1" else -0.5
    u, v = np.meshgrid((x + r + lo) / w, (y + r + lo) / h, indexing="xy")
    dy = lens_rays(lens, u, v, z.ZRT_LENS_PINHOLE)[1][..., 1]
    col = sky(dy).reshape(-1, 3)
    return col.mean(0), col.var(0)


# ---- ambient occlusion on (e) ---------------------------------------------------------------

def ao_expected(cam, w, h, tri, centre, radius):
    """1 - form factor at each pixel-centre ray's hit point on the floor triangle (u = x / w, v =
    y / h: zrt.h "ambient occlusion"), float64[h, w]; NaN where the centre ray misses the floor
    or meets the sphere first."""
    n = tri_normal(*tri)
    out = np.full((h, w), np.nan)
    org = vec(cam.origin)
    for y in range(h):
        for x in range(w):
            d = unit(vec(cam.lower_left_corner) + vec(cam.horizontal) * (x / w) + vec(cam.vertical) * (y / h) - org)
            if d @ n < 0 and sphere_t(org, d, np.asarray(centre, np.float64), radius) is None:
                p = org + d * (float((f32(tri[0]) - org) @ n) / float(d @ n))
                out[y, x] = 1.0 - occlusion_form(p, n, centre, radius)
    return out
