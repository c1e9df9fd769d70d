"""Four small BVH scenes around the edges of Material.scatter and the texture lookup.

Test infrastructure: used by tests/test_shading_scenes.py (CPU: proves that the
primary rays of each scene reach the branches it is named for) and
tests/test_gpu_shading_edges.py (GPU: every sampling loop against the oracle).
Built through ctypes as tests/lean_scenes.py builds its mound; every scene is that
mound (12 triangles) over the ground sphere plus a few spheres, 14 - 26
primitives: more than 10, so the BVH is used, and few enough for the oracle to
render a frame in about a second.

  "glass-inside"  the camera sits inside a glass sphere (r = 1, ior 1.5), 0.8 r
                  off its centre and looking across the offset: every primary ray
                  meets the glass from the back (front_face false, ratio = ior),
                  about half of them past the critical angle (material.zig:116)
  "bubbles"       seen from outside: a sphere with ior 0.6667 (front hits with
                  ratio 1.5: total internal reflection at a first, front hit), a
                  sphere with ior 1.0, a hollow shell (r = 0.5, ior 1.5, and
                  r = -0.45 at the same centre, which rays refracted into the
                  glass meet from the back); the mound's facets are glass, metal
                  with an image texture and Lambertian with an image texture in turn
  "wraps"         four images - 1 x 1 and 5 x 3 with f32 values, 1 x 7 and 8 x 2
                  with values k / 255, so both device texel stores hold two images
                  and the second of each starts at an offset - under Lambertian and
                  metal materials on spheres and on the mound, with the (u, v)
                  offsets OFFSETS: every arm of the wrap (texture.zig:52-74), the
                  V wrap that tests uu_first (:66) included
  "poles"         a "wraps" material on a sphere whose lowest point is straight
                  above the camera, which looks up +y at it through a narrow lens:
                  theta = acos(-outward.y) at and near 0, and the meridian where
                  atan2(-outward.z, -outward.x) jumps (sphere.zig:47-50) across
                  the frame; the scattered paths fall back onto the "wraps" scene
"""
import ctypes as C
import math

import numpy as np

import zraytrace_amd as z
from zraytrace_amd import _ffi

import lean_scenes as L

NAMES = ("glass-inside", "bubbles", "wraps", "poles")
OFFSETS = ((-0.3, 0.35), (-0.3, -0.2), (1.25, 0.9), (0.0, 0.0))
NO_TEXTURE = 0xFFFFFFFF  # a dielectric's texture index: read by nobody

GLASS_CENTER, GLASS_R = (1.6, 1.3, -2.2), 1.0
BUBBLE_R = 0.5
SHELL_CENTER, SHELL_INNER_R = (0.75, 1.0, 0.2), -0.45
POLE_CENTER, POLE_R = (0.0, 3.0, 0.0), 2.0


def images():
    """The four images of "wraps" as float32[h, w, 3] (row 0 = bottom): 1 x 1 and 5 x 3
    of arbitrary f32 values, 1 x 7 and 8 x 2 of values k / 255 (what png_image.zig:76-89
    produces); the texels of one image all differ, so a wrong texel shows."""
    rng = np.random.default_rng(23)
    f1 = rng.random((1, 1, 3), dtype=np.float32)
    f2 = rng.random((3, 5, 3), dtype=np.float32)
    k3 = rng.integers(0, 256, (7, 1, 3)).astype(np.float32) / np.float32(255.0)
    k4 = rng.integers(0, 256, (2, 8, 3)).astype(np.float32) / np.float32(255.0)
    return [np.ascontiguousarray(a, np.float32) for a in (f1, f2, k3, k4)]


# textures: ("c", rgb) or ("i", image, offsets); materials: ("L" | "M", texture) or ("D", ior)
_GROUND = ("c", (0.2, 0.7, 0.25))
WRAP_TEXTURES = [_GROUND,
                 ("i", 1, OFFSETS[0]), ("i", 1, OFFSETS[1]), ("i", 3, OFFSETS[1]), ("i", 3, OFFSETS[0]),
                 ("i", 2, OFFSETS[1]), ("i", 2, OFFSETS[2]), ("i", 0, OFFSETS[3]), ("i", 1, OFFSETS[2]),
                 ("i", 3, OFFSETS[3]), ("i", 0, OFFSETS[0]), ("i", 2, OFFSETS[0])]
WRAP_MATERIALS = [("L", 0),
                  ("L", 1), ("M", 2), ("L", 3), ("M", 4), ("L", 5), ("M", 6),  # the mound's facets in turn
                  ("M", 1), ("L", 2), ("M", 3), ("L", 4), ("M", 5), ("L", 7),  # spheres
                  ("M", 8), ("L", 9), ("M", 10), ("L", 11)]
# the spheres of "wraps" (and the backdrop of "poles"): centre, radius, material - eight in a
# ring round the mound and two above it
WRAP_SPHERES = [((1.45 * math.cos(k * math.pi / 4.0 + 0.2), -0.14 + 0.1 * (k % 2),
                  1.45 * math.sin(k * math.pi / 4.0 + 0.2)), 0.36, 7 + k) for k in range(8)]
WRAP_SPHERES += [((-0.7, 1.0, 0.3), 0.35, 15), ((0.7, 1.0, 0.3), 0.35, 16)]
# the mound's materials in "wraps": its six faces 1 .. 6, the flap at each face's foot another
WRAP_MOUND = (1, 4, 2, 5, 4, 6, 3, 4, 5, 1, 6, 2)
# a wall behind the mound, facing the camera of "wraps": two large triangles, metal and
# Lambertian with offsets (-0.3, -0.2), whose barycentric (u, v) cover the whole triangle
# (leaning back: a triangle in a plane z = const has a box of no depth, which aabb.zig:109-127 never enters)
WRAP_WALL = [((-1.7, -0.5, 1.7), (-1.7, 1.9, 2.1), (1.7, -0.5, 1.7), 2),
             ((1.7, 1.9, 2.1), (1.7, -0.5, 1.7), (-1.7, 1.9, 2.1), 3)]


def _spec(name):
    """(spheres, triangles, materials, textures, images) of a scene; a sphere is
    (centre, radius, material), a triangle (a, b, c, material)."""
    ground = (0.0, -0.5 - L.GROUND_R, 0.0)
    mound = L._mound()
    if name == "glass-inside":
        texs = [_GROUND, ("c", (0.8, 0.8, 0.85)), ("c", (0.7, 0.3, 0.2)), ("c", (0.9, 0.9, 0.2))]
        mats = [("L", 0), ("M", 1), ("L", 2), ("M", 3), ("D", 1.5)]
        tris = [t + (1 + i % 3,) for i, t in enumerate(mound)]
        return [(ground, L.GROUND_R, 0), (GLASS_CENTER, GLASS_R, 4)], tris, mats, texs, []
    if name == "bubbles":
        texs = [_GROUND, ("i", 1, (0.25, 0.1)), ("i", 3, (0.19, 0.1))]
        mats = [("L", 0), ("D", 1.5), ("M", 1), ("L", 2), ("D", 0.6667), ("D", 1.0)]
        spheres = [(ground, L.GROUND_R, 0), ((-0.75, 1.0, 0.2), BUBBLE_R, 4), ((0.0, 1.45, 0.9), BUBBLE_R, 5),
                   (SHELL_CENTER, 0.5, 1), (SHELL_CENTER, SHELL_INNER_R, 1)]
        tris = [t + (1 + i % 3,) for i, t in enumerate(mound)]  # glass, image metal, image Lambertian in turn
        return spheres, tris, mats, texs, images()
    spheres = [(ground, L.GROUND_R, 0)] + WRAP_SPHERES
    if name == "poles":
        spheres.append((POLE_CENTER, POLE_R, 8))  # Lambertian, the 5 x 3 f32 image at (-0.3, -0.2)
    tris = [t + (WRAP_MOUND[i],) for i, t in enumerate(mound)] + WRAP_WALL
    return spheres, tris, WRAP_MATERIALS, WRAP_TEXTURES, images()


def scene(name):
    """The zrt_scene of one of NAMES (keep the returned object alive): the mound's
    triangles first, then the spheres."""
    assert name in NAMES
    spheres, tris, mat_spec, tex_spec, imgs = _spec(name)
    texs = (_ffi.Texture * len(tex_spec))()
    for i, t in enumerate(tex_spec):
        if t[0] == "c":
            texs[i] = _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(*t[1]), 0.0, 0.0)
        else:
            texs[i] = _ffi.Texture(_ffi.ZRT_TEX_IMAGE, t[1], _ffi.Vec3(0.0, 0.0, 0.0), t[2][0], t[2][1])
    mats = (_ffi.Material * len(mat_spec))()
    for i, m in enumerate(mat_spec):
        if m[0] == "D":
            mats[i] = _ffi.Material(_ffi.ZRT_MAT_DIELECTRIC, NO_TEXTURE, m[1])
        else:
            mats[i] = _ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN if m[0] == "L" else _ffi.ZRT_MAT_METAL, m[1], 0.0)
    if imgs:
        image_array = (_ffi.Image * len(imgs))(*[_ffi.Image(a.shape[1], a.shape[0],
                                                            a.ctypes.data_as(C.POINTER(C.c_float))) for a in imgs])
        image_ptr = C.cast(image_array, C.POINTER(_ffi.Image))
    else:
        image_array, image_ptr = None, C.cast(None, C.POINTER(_ffi.Image))
    n = len(tris) + len(spheres)
    prims = (_ffi.Prim * n)()
    for i, (a, b, c, material) in enumerate(tris):
        prims[i].kind = _ffi.ZRT_PRIM_TRIANGLE
        prims[i].material = material
        prims[i].a, prims[i].b, prims[i].c = _ffi.Vec3(*a), _ffi.Vec3(*b), _ffi.Vec3(*c)
    for i, (center, radius, material) in enumerate(spheres, len(tris)):
        prims[i].kind = _ffi.ZRT_PRIM_SPHERE
        prims[i].material = material
        prims[i].center = _ffi.Vec3(*center)
        prims[i].radius = radius
    s = _ffi.Scene(prims, n, len(mat_spec), mats, texs, len(tex_spec), len(imgs), image_ptr)
    s._keep = (prims, mats, texs, image_array, imgs)
    return s


def camera(name):
    if name == "glass-inside":  # 0.8 r above the glass sphere's centre, looking across that offset at the mound
        cx, cy, cz = GLASS_CENTER
        return z.camera_init((cx, cy + 0.8 * GLASS_R, cz), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 50.0, 1.0)
    if name == "bubbles":
        return z.camera_init((0.0, 1.0, -3.2), (0.0, 0.45, 0.0), (0.0, 1.0, 0.0), 37.0, 1.0)
    if name == "poles":  # under the pole sphere's lowest point (0, 1, 0), looking straight up at it
        return z.camera_init((0.0, 0.62, 0.0), POLE_CENTER, (0.0, 0.0, 1.0), 1.5, 1.0)
    return z.camera_init((0.3, 1.6, -3.4), (0.0, 0.1, 0.0), (0.0, 1.0, 0.0), 38.0, 1.0)


_CACHE = {}


def get(name):
    """(scene object, zrt_scene pointer, camera), built once per name."""
    if name not in _CACHE:
        s = scene(name)
        _CACHE[name] = (s, C.pointer(s), camera(name))
    return _CACHE[name]


# ---- what a primary ray meets: f32 restatements for tests/test_shading_scenes.py ------

def primary_rays(cam, w=24, h=24):
    """The pixel-centre rays of a w x h frame (raytrace.zig:173-175 with both random
    floats 0.5; camera.zig:46-51): (origins[n, 3], directions[n, 3]) in f32, row-major
    from the bottom row."""
    def v3(v):
        return np.array([v.x, v.y, v.z], np.float32)
    o, llc, hor, ver = v3(cam.origin), v3(cam.lower_left_corner), v3(cam.horizontal), v3(cam.vertical)
    u = (np.arange(w, dtype=np.float32) / np.float32(w))[None, :, None]
    v = (np.arange(h, dtype=np.float32) / np.float32(h))[:, None, None]
    d = (((llc + hor * u).astype(np.float32) + (ver * v).astype(np.float32)).astype(np.float32) - o).astype(np.float32)
    d = d.reshape(-1, 3)
    return np.repeat(o[None], len(d), 0), d


def unit(d):
    """Ray.init's normalisation (vector.zig:88-92) in f32."""
    d = np.asarray(d, np.float32)
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)
    return (d / length[:, None]).astype(np.float32)


def dot(a, b):
    """Vec3.dot in f32: (x x' + y y') + z z'."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    xy = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]).astype(np.float32)
    return (xy + a[..., 2] * b[..., 2]).astype(np.float32)


def dielectric_branch(d_unit, outward, ior):
    """hit_record.zig:28-41 and material.zig:111-116 in f32 for a dielectric hit:
    (front_face, cannot_refract = ratio * sin_theta > 1)."""
    one = np.float32(1.0)
    front = not dot(d_unit, outward) > 0.0
    normal = np.asarray(outward, np.float32) if front else -np.asarray(outward, np.float32)
    ratio = one / np.float32(ior) if front else np.float32(ior)
    cos_theta = min(dot(-np.asarray(d_unit, np.float32), normal), one)
    sin_theta = np.sqrt(np.float32(one - np.float32(cos_theta * cos_theta)), dtype=np.float32)
    return front, bool(np.float32(ratio * sin_theta) > one)


def refract(d_unit, normal, ratio):
    """Vec3.refract (vector.zig:134-139) in f32."""
    d_unit, normal, ratio = np.asarray(d_unit, np.float32), np.asarray(normal, np.float32), np.float32(ratio)
    cos_theta = min(dot(-d_unit, normal), np.float32(1.0))
    perp = ((d_unit + normal * cos_theta).astype(np.float32) * ratio).astype(np.float32)
    par = normal * -np.sqrt(np.abs(np.float32(1.0) - dot(perp, perp)), dtype=np.float32)
    return (perp + par).astype(np.float32)


def triangle_uv(a, b, c, o, d_unit):
    """Triangle.hit's texture coordinates (triangle.zig:53-60) in f32."""
    a, b, c, o, d = (np.asarray(x, np.float32) for x in (a, b, c, o, d_unit))
    e1, e2 = (b - a).astype(np.float32), (c - a).astype(np.float32)

    def cross(p, q):
        return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]], np.float32)
    inv_det = np.float32(1.0) / -dot(d, cross(e1, e2))
    dao = cross((o - a).astype(np.float32), d)
    return np.float32(dot(e2, dao) * inv_det), np.float32(-dot(e1, dao) * inv_det)


def wrap_arms(u, v, u_off, v_off):
    """The arms ImageTexture.albedo takes (texture.zig:54-68) in f32, as a set of names."""
    u, v, u_off, v_off = (np.float32(x) for x in (u, v, u_off, v_off))
    uu_first = np.float32(np.float32(np.float32(1.0) - u) + u_off)
    vv_first = np.float32(v + v_off)
    arms = set()
    if uu_first > 1.0:
        arms.add("uu_first > 1")
    elif uu_first < 0.0:
        arms.add("uu_first < 0")
    if vv_first > 1.0:
        arms.add("vv_first > 1")
    elif uu_first < 0.0:
        arms.add("quirk")
        if np.float32(vv_first + np.float32(1.0)) > 1.0:
            arms.add("quirk past 1")
    elif vv_first < 0.0:
        arms.add("vv_first < 0 kept")
    return arms


def classify(O, name, w=24, h=24):
    """What the w x h pixel-centre primary rays of a scene meet, with the oracle's
    closest hit (O.trace through the BVH), its sphere hit record (O.sphere_hit) and the
    restatements above: a dict class name -> number of rays (see
    tests/test_shading_scenes.py for the classes each scene must reach)."""
    from collections import Counter
    s, view, cam = get(name)
    o, d = primary_rays(cam, w, h)
    t, prim = O.trace(view, True, o, d)
    du = unit(d)
    n = Counter(rays=len(d), hits=int((prim >= 0).sum()))
    inf = float("inf")
    for k in np.flatnonzero(prim >= 0):
        p = s.prims[int(prim[k])]
        m = s.materials[p.material]
        if p.kind == _ffi.ZRT_PRIM_SPHERE:
            center = (p.center.x, p.center.y, p.center.z)
            ok, rec = O.sphere_hit(center, p.radius, o[k], d[k], 0.001, inf)
            assert ok and rec[6] == t[k]
            u, v = rec[7], rec[8]
            outward = ((rec[0:3] - np.array(center, np.float32)).astype(np.float32)
                       * (np.float32(1.0) / np.float32(p.radius))).astype(np.float32)
            shape = "sphere"
        else:
            a, b, c = ((q.x, q.y, q.z) for q in (p.a, p.b, p.c))
            ok, rec = O.triangle_hit(a, b, c, o[k], d[k], 0.001, inf)
            assert ok and rec[6] == t[k] and rec[7] == 1.0  # (single sided: always the front)
            u, v = triangle_uv(a, b, c, o[k], du[k])
            outward = rec[3:6]
            shape = "triangle"
        if m.kind == _ffi.ZRT_MAT_DIELECTRIC:
            front, tir = dielectric_branch(du[k], outward, m.index_of_refraction)
            n[f"dielectric {shape}"] += 1
            n[f"dielectric {'front' if front else 'back'} {'TIR' if tir else 'Schlick'}"] += 1
            if name == "bubbles" and shape == "sphere" and p.radius == 0.5 and front and not tir:
                # the hollow shell: where the refracted ray goes (when Schlick's draw lets it)
                d2 = refract(du[k], outward, np.float32(1.0) / np.float32(m.index_of_refraction))
                ok2, rec2 = O.sphere_hit(SHELL_CENTER, SHELL_INNER_R, rec[0:3], d2, 0.001, inf)
                ok3, rec3 = O.sphere_hit(SHELL_CENTER, 0.5, rec[0:3], d2, 0.001, inf)
                if ok2 and (not ok3 or rec2[6] < rec3[6]):
                    out2 = ((rec2[0:3] - np.array(SHELL_CENTER, np.float32)).astype(np.float32)
                            * (np.float32(1.0) / np.float32(SHELL_INNER_R))).astype(np.float32)
                    front2, tir2 = dielectric_branch(unit(d2[None])[0], out2, m.index_of_refraction)
                    n[f"shell inside {'front' if front2 else 'back'}"] += 1
                    n[f"shell inside {'TIR' if tir2 else 'Schlick'}"] += 1
            continue
        tex = s.textures[m.texture]
        if tex.kind != _ffi.ZRT_TEX_IMAGE:
            continue
        kind = "metal" if m.kind == _ffi.ZRT_MAT_METAL else "lambertian"
        n[f"image {kind} {shape}"] += 1
        n[f"image {tex.image}"] += 1
        for arm in wrap_arms(u, v, tex.u_offset, tex.v_offset):
            n[arm] += 1
        if shape == "sphere" and p.radius == POLE_R:
            theta = np.float32(v) * np.float32(np.pi)
            n["pole"] += 1
            if theta < 2.0 ** -10:
                n["theta < 2^-10"] += 1
            if np.isnan(v):
                n["theta NaN"] += 1
            if u < 0.125:
                n["seam, u near 0"] += 1
            if u > 0.875:
                n["seam, u near 1"] += 1
    return dict(n)
