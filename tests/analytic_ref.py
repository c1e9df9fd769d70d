"""Scenes whose radiance has a closed form, and the closed forms, in float64.

Test infrastructure: used by tests/test_analytic_ref.py (CPU: the oracle against the forms,
and the forms' power against named wrong models) and tests/test_gpu_analytic.py (GPU: every
kernel that produces radiance against the same forms).  Nothing here reads oracle.c or a
kernel: every formula is derived from the reference's source lines, cited beside it, in
plain numpy float64 - no traversal, no BVH, no sampler, no f32 emulation.

  sky(d_y) = (1 - t) white + t (0.5, 0.7, 1.0), t = 0.5 (d_y + 1)     (raytrace.zig:53-58)
           = SKY_A + SKY_B d_y: linear in the unit direction's y.

A Case holds a scene (built through ctypes as tests/shading_scenes.py builds its scenes),
one ray (origin, target: the degenerate camera of tests/radiance_ref.py maps every pixel
onto it), max_depth, and per channel the expected mean and the exact variance of ONE
sample's colour; where they have a closed form, the expected Progress counters per sample
(raytrace.zig:62-100) with their variances.  mean(model) gives the mean under a named
wrong model (MODELS), for the power checks.

The acceptance rule (accept): |mean - expected| <= 5 sqrt(var / N) + floor, with var from
here, never from the output under test.
"""
import ctypes as C
import functools
import math

import numpy as np

from zraytrace_amd import _ffi

WHITE, BLUE = np.array([1.0, 1.0, 1.0]), np.array([0.5, 0.7, 1.0])
SKY_A, SKY_B = (WHITE + BLUE) / 2, (BLUE - WHITE) / 2
COUNTERS = ("rays", "reflections", "background_hits", "recursion_depth_hits")
MODELS = ("uniform-hemisphere", "r0-squared", "eta-swapped", "depth+1", "depth-1", "jitter-0-1", "no-occluder")
NO_TEXTURE = 0xFFFFFFFF
T_MIN = 0.001  # raytrace.zig:71


def sky(dy):
    return SKY_A + SKY_B * np.asarray(dy, np.float64)[..., None]


def f32(v):
    """The float64 value of v rounded to f32: what the scene and the ray really hold."""
    return np.asarray(v, np.float32).astype(np.float64)


def unit(v):
    v = np.asarray(v, np.float64)
    return v / math.sqrt(float(v @ v))


def chunk_floor(n_samples, chunk=32):
    """The f32 rounding of a chunked sum of values <= 1, as a bound on the mean:
    (chunk + n_chunks + 2) 2^-24."""
    return (chunk + -(-n_samples // chunk) + 2) * 2.0 ** -24


def accept(mean, expected, var, n, floor):
    """(ok per channel, z = deviation / standard error where var > 0 else 0)."""
    mean, expected, var = (np.asarray(a, np.float64) for a in (mean, expected, var))
    se = np.sqrt(var / n)
    dev = np.abs(mean - expected)
    with np.errstate(all="ignore"):
        zs = np.where(se > 0, dev / se, 0.0)
    return dev <= 5.0 * se + floor, zs


# ---- scenes -------------------------------------------------------------------------------

def build_scene(spheres, tris, mats):
    """A zrt_scene (keep the object alive).  spheres: (centre, radius, material); tris:
    (a, b, c, material), first in the list; mats: ("L" | "M", rgb) or ("D", ior), every
    material with a colour texture of its own."""
    texs = (_ffi.Texture * len(mats))()
    ms = (_ffi.Material * len(mats))()
    for i, m in enumerate(mats):
        if m[0] == "D":
            texs[i] = _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.0, 0.0, 0.0), 0.0, 0.0)
            ms[i] = _ffi.Material(_ffi.ZRT_MAT_DIELECTRIC, NO_TEXTURE, m[1])
        else:
            texs[i] = _ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(*[float(c) for c in m[1]]), 0.0, 0.0)
            ms[i] = _ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN if m[0] == "L" else _ffi.ZRT_MAT_METAL, i, 0.0)
    n = len(tris) + len(spheres)
    prims = (_ffi.Prim * n)()
    for i, (a, b, c, material) in enumerate(tris):
        prims[i].kind, prims[i].material = _ffi.ZRT_PRIM_TRIANGLE, material
        prims[i].a, prims[i].b, prims[i].c = (_ffi.Vec3(*[float(x) for x in v]) for v in (a, b, c))
    for i, (centre, radius, material) in enumerate(spheres, len(tris)):
        prims[i].kind, prims[i].material = _ffi.ZRT_PRIM_SPHERE, material
        prims[i].center, prims[i].radius = _ffi.Vec3(*[float(x) for x in centre]), float(radius)
    s = _ffi.Scene(prims, n, len(mats), ms, texs, len(mats), 0, C.cast(None, C.POINTER(_ffi.Image)))
    s._keep = (prims, ms, texs)
    return s


PAD_MAT = ("L", (1.0, 0.0, 0.0))  # what no path may reach: red, so that a reached one would show


def padding(centre, spread, radius, material, axis=None, n=12):
    """n tiny spheres: scattered within `spread` of centre, or (axis given) strung along
    +-axis from centre at distances spread (1 + k / 4): more than 10 primitives make the
    reference build its BVH (raytrace.zig:127)."""
    centre = np.asarray(centre, np.float64)
    out = []
    for k in range(n):
        if axis is None:
            off = spread * np.array([math.cos(1.0 + 2.3 * k), math.sin(0.7 + 1.9 * k), math.cos(2.0 + 3.1 * k)]) / 1.8
        else:
            off = np.asarray(axis) * (spread * (1.0 + (k // 2) / 4.0) * (1 if k % 2 else -1))
        out.append((tuple(centre + off), radius, material))
    return out


class Case:
    def __init__(self, name, spheres, tris, mats, o, tgt, depth, mean, var, counters=None, counter_var=None,
                 pad=None):
        self.name, self.spheres, self.tris, self.mats, self.depth = name, spheres, tris, list(mats), depth
        self.o, self.tgt = np.asarray(o, np.float32), np.asarray(tgt, np.float32)
        assert not (np.signbit(self.tgt) & (self.tgt == 0)).any()
        self._mean, self.var = mean, np.asarray(var, np.float64) * np.ones(3)
        self.counters, self.counter_var, self.pad = counters, counter_var, pad
        self.zero_variance = not self.var.any()
        self.extra_floor, self.cpu_side, self.counters_of = 0.0, 64, None
        self.exact_counters = counters is not None and (counter_var is None or not any(counter_var.values()))

    def mean(self, model=None):
        return np.asarray(self._mean(model), np.float64) * np.ones(3)

    @functools.lru_cache(maxsize=None)
    def scene(self, bvh=False):
        """(scene object, pointer to it).  bvh: with the case's unreachable padding."""
        if not bvh:
            s = build_scene(self.spheres, self.tris, self.mats)
        else:
            assert self.pad is not None, f"{self.name} has no padded variant"
            s = build_scene(self.spheres + self.pad(len(self.mats)), self.tris, self.mats + [PAD_MAT])
            assert s.n_prims > 10
        return s, C.pointer(s)

    def ray(self):
        """(origin, direction) as the query is fed them: f32, direction = f32(tgt - o)."""
        return self.o, self.tgt - self.o


def _ray64(o, tgt):
    """The ray the reference traces, in float64, from the f32 origin and target."""
    o, tgt = np.asarray(o, np.float32), np.asarray(tgt, np.float32)
    return o.astype(np.float64), unit((tgt - o).astype(np.float64))


def sphere_t(o, d, centre, radius):
    """Sphere.hit's t (sphere.zig:31-71): the first root in (T_MIN, inf), or None."""
    oc = o - centre
    hb = float(oc @ d)
    disc = hb * hb - (float(oc @ oc) - radius * radius)
    if disc < 0:
        return None
    for t in (-hb - math.sqrt(disc), -hb + math.sqrt(disc)):
        if t > T_MIN:
            return t
    return None


def reflect(v, n):
    return v - n * (2.0 * float(v @ n))  # vector.zig:129-131


# ---- a. Lambertian: unit(n + u), u uniform on the sphere, is cosine-distributed about n -----

def lambert_moments(ny, cos_cut=1.0):
    """Of d = unit(n + randomUnitVector) (material.zig:71-76; sample.zig:47-61: z = +-r1 uniform
    in (-1, 1), phi uniform: uniform on the sphere, so d has density cos(theta) / pi about n)
    restricted to cos(theta) < cos_cut: (P, E[d_y; .], E[d_y^2; .]).  With c = cos(theta) of
    density 2c and d_y = c n_y + sqrt(1 - c^2) cos(phi) sqrt(1 - n_y^2): E_phi[d_y] = c n_y,
    E_phi[d_y^2] = c^2 n_y^2 + (1 - c^2)(1 - n_y^2) / 2.  Whole lobe: 1, (2/3) n_y, (1 + n_y^2) / 4."""
    c2, c3, c4 = cos_cut ** 2, cos_cut ** 3, cos_cut ** 4
    return c2, (2.0 / 3.0) * ny * c3, ny * ny * c4 / 2 + (1 - ny * ny) / 2 * (c2 - c4 / 2)


def lambert_mean_var(rho, ny, cos_cut=1.0, model=None):
    """Mean and variance of rho * sky(d_y) * [cos(theta) < cos_cut] per channel."""
    rho = np.asarray(rho, np.float64)
    m0, m1, m2 = lambert_moments(ny, 1.0 if model == "no-occluder" else cos_cut)
    if model == "uniform-hemisphere":  # c uniform on (0, 1): P = C, E[d_y; .] = n_y C^2 / 2 (whole: n_y / 2)
        m0, m1 = cos_cut, ny * cos_cut ** 2 / 2
    mean = rho * (SKY_A * m0 + SKY_B * m1)
    return mean, rho * rho * (SKY_A ** 2 * m0 + 2 * SKY_A * SKY_B * m1 + SKY_B ** 2 * m2) - mean * mean


def _depth(depth, model):
    return depth + (model == "depth+1") - (model == "depth-1")


RHO = (0.8, 0.6, 0.4)
LAMBERT_NORMALS = {"up": (0.0, 1.0, 0.0), "down-ish": (0.0, -0.8, 0.6), "equator": (0.6, 0.0, -0.8),
                   "generic": (0.48, 0.6, 0.64)}


LAMBERT_PADDED = (("up", 2), ("generic", 2))  # the cases that also run BVH-padded


def lambert_sphere(which, depth=2):
    """A unit sphere of albedo RHO alone, met at the point with normal n: rho sky((2/3) n_y) at
    any depth >= 2, black at 1; 2 rays, 1 reflection, 1 background hit per sample, exactly."""
    n = np.array(LAMBERT_NORMALS[which])
    side = unit(np.cross(n, (0.3, 0.2, 1.0)))
    o, tgt = n * 4.0 + side * 1.5, n
    o, d = _ray64(o, tgt)
    ny = (o + d * sphere_t(o, d, np.zeros(3), 1.0))[1]  # the normal the ray really meets
    var = lambert_mean_var(RHO, ny)[1]

    def m(model):
        return lambert_mean_var(RHO, ny, model=model)[0] if _depth(depth, model) >= 2 else np.zeros(3)
    cnt = {"rays": 2, "reflections": 1, "background_hits": 1, "recursion_depth_hits": 0} if depth >= 2 else \
        {"rays": 1, "reflections": 1, "background_hits": 0, "recursion_depth_hits": 1}
    return Case(f"lambert-sphere-{which}-d{depth}", [((0, 0, 0), 1.0, 0)], [], [("L", RHO)], o, tgt, depth, m,
                var if depth >= 2 else 0.0, cnt,
                pad=(lambda mat: padding((0, 0, 0), 0.5, 0.02, mat)) if (which, depth) in LAMBERT_PADDED else None)


TILTED = ((-30.0, -9.0, -20.0), (0.0, 12.0, 40.0), (35.0, 3.0, -25.0))


def tri_normal(a, b, c):
    """Triangle.init's face_unit_normal (triangle.zig:34-37) from the f32 vertices."""
    a, b, c = f32(a), f32(b), f32(c)
    return unit(np.cross(b - a, c - a))


def lambert_triangle(front=True, depth=3):
    """A large tilted single-sided triangle (triangle.zig:55-67: det = -d . face_normal >= 1e-6
    is the front).  From the front rho sky((2/3) n_y): the scattered ray has d . n > 0 and
    cannot meet the triangle again.  From the back the ray sees the sky through it."""
    n = tri_normal(*TILTED)
    p = (np.array(TILTED[0]) + TILTED[1] + TILTED[2]) / 3.0
    o = p + (n * 3.0 + np.array([1.0, 0.5, -0.7])) * (1 if front else -1)
    o64, d = _ray64(o, p)
    assert (d @ n < -0.5) == front
    if front:
        var = lambert_mean_var(RHO, n[1])[1]
        return Case("lambert-triangle-front", [], [TILTED + (0,)], [("L", RHO)], o, p, depth,
                    lambda model: lambert_mean_var(RHO, n[1], model=model)[0], var,
                    {"rays": 2, "reflections": 1, "background_hits": 1, "recursion_depth_hits": 0})
    return Case("lambert-triangle-back", [], [TILTED + (0,)], [("L", RHO)], o, p, depth, lambda model: sky(d[1]), 0.0,
                {"rays": 1, "reflections": 0, "background_hits": 1, "recursion_depth_hits": 0})


# ---- b. metal: rho sky(reflect(d, n)_y), no variance (material.zig:87-96) --------------------

METAL_RHO = (0.9, 0.5, 0.7)


def metal_sphere():
    o, tgt = (2.5, 1.5, -3.0), (0.3, 0.45, -0.2)
    o64, d = _ray64(o, tgt)
    n = o64 + d * sphere_t(o64, d, np.zeros(3), 1.0)
    r = reflect(d, n)
    assert r @ n > 0
    return Case("metal-sphere", [((0, 0, 0), 1.0, 0)], [], [("M", METAL_RHO)], o, tgt, 5,
                lambda model: (np.array(METAL_RHO) * sky(r[1])) if _depth(5, model) >= 2 else np.zeros(3), 0.0,
                {"rays": 2, "reflections": 1, "background_hits": 1, "recursion_depth_hits": 0},
                pad=lambda mat: padding((0, 0, 0), 0.5, 0.02, mat))


# ---- c. dielectric sphere: a walk in the plane of incidence -------------------------------

def reflectance(cosine, ratio, model=None):
    """material.zig:125-128: r0 = (1 - ratio) / (1 + ratio), NOT squared; the comparison with
    a float in [0, 1) (material.zig:117) makes it a probability clipped to [0, 1]."""
    r0 = (1.0 - ratio) / (1.0 + ratio)
    if model == "r0-squared":
        r0 = r0 * r0
    return min(max(r0 + (1.0 - r0) * (1.0 - cosine) ** 5, 0.0), 1.0)


def refract(v, n, ratio):
    """vector.zig:134-139."""
    cos_theta = min(float(-v @ n), 1.0)
    perp = (v + n * cos_theta) * ratio
    return perp - n * math.sqrt(abs(1.0 - float(perp @ perp)))


def dielectric_walk(o, d, ior, depth, model=None):
    """Every way rayColor (raytrace.zig:62-100) can go along a ray at a unit dielectric sphere
    at the origin, alone in the scene: [(probability, colour, counters in COUNTERS' order)].
    Each scatter (material.zig:109-123; front_face and the normal: hit_record.zig:28-41)
    branches into reflect (probability R, 1 if cannot_refract) and refract; a branch that
    leaves the sphere ends on the sky at the next ray, so the tree is a comb of <= 2 depth leaves."""
    leaves = []

    def go(o, d, depth, prob, cnt):
        assert len(leaves) < 4096
        if depth <= 0:
            leaves.append((prob, np.zeros(3), cnt + np.array([0, 0, 0, 1])))
            return
        cnt = cnt + np.array([1, 0, 0, 0])
        t = sphere_t(o, d, np.zeros(3), 1.0)
        if t is None:
            leaves.append((prob, sky(d[1]), cnt + np.array([0, 0, 1, 0])))
            return
        p = o + d * t
        front = not float(d @ p) > 0.0
        n = p if front else -p
        ratio = (1.0 / ior if front else ior) if model != "eta-swapped" else (ior if front else 1.0 / ior)
        cos_theta = min(float(-d @ n), 1.0)
        sin_theta = math.sqrt(1.0 - cos_theta * cos_theta)
        r = 1.0 if ratio * sin_theta > 1.0 else reflectance(cos_theta, ratio, model)
        cnt = cnt + np.array([0, 1, 0, 0])
        if r > 0:
            go(p, unit(reflect(d, n)), depth - 1, prob * r, cnt)
        if r < 1:
            go(p, unit(refract(d, n, ratio)), depth - 1, prob * (1 - r), cnt)

    go(o, d, _depth(depth, model), 1.0, np.zeros(4, np.int64))
    return leaves


def moments(leaves):
    """(mean colour, colour variance, mean counters, counter variances) of the discrete distribution."""
    p = np.array([l[0] for l in leaves])
    assert abs(p.sum() - 1.0) < 1e-12
    col, cnt = np.array([l[1] for l in leaves]), np.array([l[2] for l in leaves], np.float64)
    mc, mk = p @ col, p @ cnt
    if len(p) == 1:  # one way to go: no variance, exactly
        return mc, np.zeros(3), mk, np.zeros(4)
    return mc, np.maximum(p @ (col * col) - mc * mc, 0.0), mk, np.maximum(p @ (cnt * cnt) - mk * mk, 0.0)


GLASS_AXIS = unit((0.6, -0.35, -0.72))                         # the ray's direction
GLASS_SIDE = unit(np.cross(GLASS_AXIS, (0.3, 1.0, 0.2)))       # the impact parameter's axis
GLASS_OFF = unit(np.cross(GLASS_AXIS, GLASS_SIDE))             # the plane of incidence's normal
IMPACTS = {"centre": 0.0, "near-centre": 0.1, "generic": 0.55, "grazing": 0.9}
# (ior, impact, max_depth): every ior at a near-centre, a generic and a grazing ray, every depth
# of 1, 2, 3, 50; ior 0.6667 reflects inside (r0 = +0.2 at a back hit: the series has many terms)
# and, grazing, cannot refract at its first, front hit (1.5 * 0.9 > 1)
GLASS = [(1.5, "near-centre", 50), (1.5, "generic", 3), (1.5, "grazing", 2), (1.5, "generic", 1),
         (1.0, "centre", 50), (1.0, "generic", 3), (1.0, "grazing", 50),
         (2.4, "near-centre", 3), (2.4, "generic", 50), (2.4, "grazing", 2),
         (0.6667, "near-centre", 2), (0.6667, "generic", 50), (0.6667, "generic", 3), (0.6667, "grazing", 50)]


GLASS_PADDED = ((1.5, "generic", 3), (1.0, "grazing", 50), (2.4, "grazing", 2), (0.6667, "generic", 50))


def dielectric_sphere(ior, impact, depth):
    b = IMPACTS[impact]
    o, tgt = GLASS_AXIS * -4.0 + GLASS_SIDE * b, GLASS_AXIS * 1.0 + GLASS_SIDE * b
    o64, d = _ray64(o, tgt)
    ior64 = float(np.float32(ior))
    mc, vc, mk, vk = moments(dielectric_walk(o64, d, ior64, depth))
    return Case(f"glass-{ior}-{impact}-d{depth}", [((0, 0, 0), 1.0, 0)], [], [("D", ior)], o, tgt, depth,
                lambda model: moments(dielectric_walk(o64, d, ior64, depth, model))[0], vc,
                dict(zip(COUNTERS, mk)), dict(zip(COUNTERS, vk)),
                pad=(lambda mat: padding((0, 0, 0), 2.5, 0.02, mat, axis=GLASS_OFF))
                if (ior, impact, depth) in GLASS_PADDED else None)


# ---- d. inside a closed Lambertian sphere: black, depth rays per sample -------------------

def closed_sphere(depth):
    """Every scattered ray meets the unit sphere again from inside at t2 = 2 cos(theta)
    (sphere.zig:56-57), theta from the inward normal with density 2 cos(theta): colour 0, depth
    rays, depth reflections and one depth hit per sample - unless t2 <= T_MIN, when Sphere.hit
    returns null and the ray leaves to the sky: probability q = (T_MIN / 2)^2 = 2.5e-7 per
    scattered ray.  At depth 1 nothing is scattered and the counts are exact; deeper, the
    leaves below give their expectations, and the escaped colour (<= rho^k) a bound on the mean."""
    q = (T_MIN / 2.0) ** 2

    def leaves(depth):
        out = [((1 - q) ** (j - 2) * q, np.array(RHO) ** (j - 1), np.array([j, j - 1, 1, 0])) for j in range(2, depth + 1)]
        return out + [((1 - q) ** max(depth - 1, 0), np.zeros(3), np.array([depth, depth, 0, 1]))]
    lv = leaves(depth)
    _, _, mk, vk = moments(lv)
    bound = sum(l[0] * l[1] for l in lv)
    c = Case(f"closed-sphere-d{depth}", [((0, 0, 0), 1.0, 0)], [], [("L", RHO)], (0.2, 0.1, -0.3), (0.5, 0.4, 0.1),
             depth, lambda model: np.zeros(3), sum(l[0] * l[1] ** 2 for l in lv) if depth > 1 else 0.0,
             dict(zip(COUNTERS, mk)), dict(zip(COUNTERS, vk)),
             pad=(lambda mat: padding((0, 0, 0), 3.0, 0.02, mat, axis=(0.0, 0.6, 0.8))) if depth < 50 else None)
    c.extra_floor = bound  # the mean lies in [0, bound]
    c.counters_of = lambda model: dict(zip(COUNTERS, moments(leaves(_depth(depth, model)))[2]))
    c.cpu_side = 64 if depth < 50 else 16  # 50 rays a sample: fewer streams on the CPU
    return c


# ---- e. a Lambertian floor under a black metal sphere -------------------------------------

FLOOR = ((0.0, 0.0, 80.0), (70.0, 0.0, -40.0), (-70.0, 0.0, -40.0))  # normal +y
OCC_R, OCC_H = 0.6, 1.0


def tilted_floor(angle):
    """FLOOR turned about the x axis: its box has a depth, so a BVH node that holds it alone
    can be entered (aabb.zig:109-127 refuses a box of no depth)."""
    c, s = math.cos(angle), math.sin(angle)
    return tuple(tuple(float(np.float32(v)) for v in (x, y * c - z * s, y * s + z * c)) for x, y, z in FLOOR)


def occlusion_form(p, n, centre, radius):
    """The cosine-weighted form factor of a sphere wholly above the horizon of (p, n):
    (r / d)^2 cos(beta), beta between n and the centre's direction; r^2 h / d^3 on a floor."""
    v = np.asarray(centre, np.float64) - p
    d2 = float(v @ v)
    assert float(v @ n) - radius > 0
    return radius * radius / d2 * float(v @ n) / math.sqrt(d2)


def occluded_floor(tilt=0.0, depth=4):
    """The floor point P straight under a black metal sphere (centre P + h n, radius r, sin^2
    alpha = r^2 / h^2): the cosine lobe about n loses the cap cos(theta) > cos(alpha), which is
    symmetric about n: mean = rho (a cos^2 alpha + (2/3) b n_y cos^3 alpha), which for n = +y is
    rho [a + (2/3) b - (a sin^2 alpha + (2/3) b (1 - cos^3 alpha))].  What meets the sphere
    returns black whatever it does next: metal of albedo 0 (material.zig:87-96)."""
    tri = tilted_floor(tilt) if tilt else FLOOR
    n = tri_normal(*tri)
    centre = f32(n * OCC_H)
    o, tgt = np.array([3.0, 0.9, 1.2]), np.zeros(3) + np.float32(0.0)
    o64, d = _ray64(o, tgt)
    assert sphere_t(o64, d, centre, OCC_R) is None and d @ n < 0
    p = o64 + d * (float((f32(tri[0]) - o64) @ n) / float(d @ n))
    v = centre - p
    cos_a = math.sqrt(1.0 - OCC_R ** 2 / float(v @ v))
    assert abs(float(unit(v) @ n) - 1.0) < 1e-6  # straight above P, up to f32
    mean, var = lambert_mean_var(RHO, n[1], cos_a)
    return Case(f"occluded-floor{'-tilted' if tilt else ''}", [(tuple(centre), OCC_R, 1)], [tri + (0,)],
                [("L", RHO), ("M", (0.0, 0.0, 0.0))], o, tgt, depth,
                lambda model: lambert_mean_var(RHO, n[1], cos_a, model)[0], var,
                pad=lambda mat: padding(centre, 0.3, 0.012, mat))


# ---- g. a periscope of flat mirrors -------------------------------------------------------

MIRROR_RHO = ((0.9, 0.8, 0.7), (0.6, 0.9, 0.8), (0.8, 0.7, 0.95))


def _mirror(centre, normal, size=3.0):
    """A triangle about centre whose face normal (b - a) x (c - a) is along `normal`."""
    n = unit(normal)
    u = unit(np.cross(n, (0.2, 0.3, 1.0)))
    v = np.cross(n, u)
    c = np.asarray(centre, np.float64)
    return tuple(tuple(float(np.float32(x)) for x in q) for q in (c + u * size, c - u * size / 2 + v * size,
                                                                  c - u * size / 2 - v * size))


def mirror_walk(o, d, tris, rhos, depth):
    """rayColor over single-sided metal triangles: (colour, mirrors met in turn).  Triangle.hit
    (triangle.zig:48-70) and Metal.scatter (material.zig:87-96) in float64."""
    att, met = np.ones(3), []
    for _ in range(depth):
        best = None
        for i, (a, b, c) in enumerate(tris):
            a, e1, e2 = f32(a), f32(b) - f32(a), f32(c) - f32(a)
            fn = np.cross(e1, e2)
            det = -float(d @ fn)
            if det < 1e-6:
                continue
            ao = o - a
            dao = np.cross(ao, d)
            u, v, t = float(e2 @ dao) / det, -float(e1 @ dao) / det, float(ao @ fn) / det
            if t > T_MIN and u >= 0 and v >= 0 and u + v <= 1 and (best is None or t < best[0]):
                best = (t, i, unit(fn))
        if best is None:
            return att * sky(d[1]), met
        t, i, n = best
        o, d = o + d * t, unit(reflect(d, n))
        assert d @ n > 0
        att, met = att * rhos[i], met + [i]
    return np.zeros(3), met


def periscope(depth=4):
    """+x onto a mirror that sends it up, one that sends it along +x again, one that sends it up
    and back to the sky: the product of the albedos times the sky at depth >= 4, black at 3."""
    tris = [_mirror((0, 0, 0), (-1.0, 1.0, 0.1)), _mirror((0.1, 4.0, 0.0), (1.0, -1.0, 0.05)),
            _mirror((4.0, 4.0, 0.2), (-1.0, 0.6, -0.3))]
    o, tgt = (-5.0, 0.1, 0.05), (0.0, 0.0, 0.0)
    tgt = tuple(np.float32(0.0) + np.float32(x) for x in tgt)
    o64, d = _ray64(o, tgt)
    col, met = mirror_walk(o64, d, tris, MIRROR_RHO, 8)
    assert met == [0, 1, 2] and col.all()
    k = min(depth, 4)
    return Case(f"periscope-d{depth}", [], [t + (i,) for i, t in enumerate(tris)], [("M", r) for r in MIRROR_RHO],
                o, tgt, depth, lambda model: mirror_walk(o64, d, tris, MIRROR_RHO, _depth(depth, model))[0], 0.0,
                {"rays": k, "reflections": min(depth, 3), "background_hits": int(depth >= 4),
                 "recursion_depth_hits": int(depth < 4)})


@functools.lru_cache(maxsize=None)
def cases():
    """Every ray case, by name."""
    out = [lambert_sphere(w) for w in LAMBERT_NORMALS] + [lambert_sphere("generic", 1), lambert_sphere("up", 50)]
    out += [lambert_triangle(True), lambert_triangle(False), metal_sphere()]
    out += [dielectric_sphere(*g) for g in GLASS]
    out += [closed_sphere(d) for d in (1, 5, 50)]
    out += [occluded_floor(), occluded_floor(0.05), periscope(4), periscope(3)]
    return {c.name: c for c in out}
