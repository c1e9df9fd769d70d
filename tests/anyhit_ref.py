"""The any-hit reference (DESIGN.md §5 "Ray queries"): what rayColor's surface loop
(raytrace.zig:71-81) returns, as `!= null`, when it is started with a caller's t_max
instead of +inf.  Test infrastructure: used by tests/test_anyhit_ref.py (CPU, pins
the two forms against each other and against oracle_trace) and by
tests/test_gpu_queries.py (GPU).

literal   bvh.zig:187-205 restated per ray, every box and primitive test a call of
          the oracle's hooks (oracle_aabb_hit / oracle_triangle_hit / oracle_sphere_hit).
leafwise  the same answer per leaf: until the first hit t_max never shrinks, so a ray
          is occluded iff some leaf whose box and all of whose ancestors' boxes pass
          hitAabb(ray, 0.001, t_max) holds a primitive that hits in (0.001, t_max).
          The box tests are vectorised over the rays in numpy f32 (aabb.zig:109-127,
          one rounding per operation, math.max / math.min as `x > y ? x : y`); hook
          calls only for the primitives of passing leaves.

The hooks call Ray.init, which normalises: they get the RAW direction (a direction
normalised beforehand moves t by an ulp on one ray in eight).
"""
import ctypes as C

import numpy as np

import hazard_rays as H
from zraytrace_amd import _ffi

F = np.float32
T_MIN = 0.001
_F3 = C.c_float * 3


def scene_struct(scene):
    """The zrt_scene behind a LoadedScene, a POINTER(Scene) or a Scene."""
    view = getattr(scene, "view", scene)
    return view.contents if hasattr(view, "contents") else view


def prim_array(scene):
    """The scene's zrt_prim array as a numpy structured array (a view)."""
    s = scene_struct(scene)
    dt = np.dtype([("kind", np.uint32), ("material", np.uint32), ("center", np.float32, 3), ("radius", np.float32),
                   ("a", np.float32, 3), ("b", np.float32, 3), ("c", np.float32, 3)])
    assert dt.itemsize == C.sizeof(_ffi.Prim)
    buf = (C.c_uint8 * (dt.itemsize * s.n_prims)).from_address(C.addressof(s.prims.contents))
    return np.frombuffer(buf, dtype=dt)


class _Hooks:
    """The oracle's hit hooks over one scene and one ray set, their arguments converted once."""

    def __init__(self, O, scene, o, d):
        self.L = O.load()
        self.pr = prim_array(scene)
        self.o = [_F3(*map(float, v)) for v in np.asarray(o, F).reshape(-1, 3)]
        self.d = [_F3(*map(float, v)) for v in np.asarray(d, F).reshape(-1, 3)]
        self.out = (C.c_float * 12)()
        self._prims = {}

    def _prim(self, i):
        if i not in self._prims:
            p = self.pr[i]
            if p["kind"] == _ffi.ZRT_PRIM_SPHERE:
                self._prims[i] = (0, _F3(*map(float, p["center"])), float(p["radius"]))
            else:
                self._prims[i] = (1, _F3(*map(float, p["a"])), _F3(*map(float, p["b"])), _F3(*map(float, p["c"])))
        return self._prims[i]

    def prim_t(self, i, ray, t_max):
        """The primitive's hit t in (0.001, t_max), or None (Sphere.hit / Triangle.hit)."""
        p = self._prim(i)
        if p[0] == 0:
            hit = self.L.oracle_sphere_hit(p[1], p[2], self.o[ray], self.d[ray], T_MIN, t_max, self.out)
        else:
            hit = self.L.oracle_triangle_hit(p[1], p[2], p[3], self.o[ray], self.d[ray], T_MIN, t_max, self.out)
        return float(self.out[6]) if hit else None

    def box(self, lo, hi, ray, t_max):
        return bool(self.L.oracle_aabb_hit(lo, hi, self.o[ray], self.d[ray], T_MIN, t_max))


def _tmax_array(t_max, n):
    if t_max is None:
        return np.full(n, np.inf, F)
    return np.ascontiguousarray(np.broadcast_to(np.asarray(t_max, F), (n,)))


def literal_t(O, scene, nodes, o, d, t_max=None):
    """bvh.zig:187-205 per ray, started at t_max: the closest hit's t (float32[n], +inf: null).
    nodes: (mins, maxs, left, right) of oracle_bvh_build; child < 0: primitive -(c + 1)."""
    mins, maxs, left, right = nodes[:4]
    n = len(o)
    tm = _tmax_array(t_max, n)
    h = _Hooks(O, scene, o, d)
    lo = [_F3(*map(float, v)) for v in mins]
    hi = [_F3(*map(float, v)) for v in maxs]

    def child(c, ray, t):
        return h.prim_t(-c - 1, ray, t) if c < 0 else node(c, ray, t)

    def node(k, ray, t):
        if not h.box(lo[k], hi[k], ray, t):
            return None
        hl = child(int(left[k]), ray, t)
        if hl is None:
            return child(int(right[k]), ray, t)
        hr = child(int(right[k]), ray, hl)
        return hr if hr is not None else hl

    out = np.full(n, np.inf, F)
    for i in range(n):
        t = node(0, i, float(tm[i]))
        if t is not None:
            out[i] = t
    return out


def literal(O, scene, nodes, o, d, t_max=None):
    """Occluded per ray (bool[n]): literal_t's result != null."""
    return np.isfinite(literal_t(O, scene, nodes, o, d, t_max))


def literal_list(O, scene, o, d, t_max=None):
    """The surface list (no BVH): some primitive's hit(ray, 0.001, t_max) is non-null."""
    n = len(o)
    tm = _tmax_array(t_max, n)
    h = _Hooks(O, scene, o, d)
    m = scene_struct(scene).n_prims
    return np.array([any(h.prim_t(k, i, float(tm[i])) is not None for k in range(m)) for i in range(n)], bool)


def loose_pass(lo, hi, o, du, t_max):
    """hitAabb(ray, 0.001, t_max) of one box for every ray (aabb.zig:109-127) in f32:
    du the normalised directions, t_max float32[n]."""
    ok = np.ones(len(o), bool)
    with np.errstate(all="ignore"):
        inv = (F(1) / du).astype(F)
        for k in range(3):
            t0 = ((F(lo[k]) - o[:, k]) * inv[:, k]).astype(F)
            t1 = ((F(hi[k]) - o[:, k]) * inv[:, k]).astype(F)
            neg = inv[:, k] < 0
            t0, t1 = np.where(neg, t1, t0), np.where(neg, t0, t1)
            tmin = np.where(t0 > F(T_MIN), t0, F(T_MIN))  # math.max(t0, t_min)
            tmax = np.where(t1 < t_max, t1, t_max)        # math.min(t1, t_max)
            ok &= ~(tmax <= tmin)
    return ok


def leafwise(O, scene, nodes, o, d, t_max=None):
    """Occluded per ray (bool[n]), per leaf: pass[child] = pass[parent] & loose(child)."""
    mins, maxs, left, right = nodes[:4]
    o = np.asarray(o, F).reshape(-1, 3)
    d = np.asarray(d, F).reshape(-1, 3)
    n = len(o)
    tm = _tmax_array(t_max, n)
    du = H.unit(d)
    h = _Hooks(O, scene, o, d)
    occluded = np.zeros(n, bool)
    passing = {0: loose_pass(mins[0], maxs[0], o, du, tm)}
    for k in range(len(left)):  # pre-order: a parent comes before its children
        pk = passing.pop(k)
        if left[k] < 0:
            prims = [-int(left[k]) - 1] + ([-int(right[k]) - 1] if right[k] != left[k] else [])
            for ray in np.nonzero(pk & ~occluded)[0]:
                t = float(tm[ray])
                occluded[ray] = any(h.prim_t(p, int(ray), t) is not None for p in prims)
        else:
            for c in (int(left[k]), int(right[k])):
                passing[c] = pk & loose_pass(mins[c], maxs[c], o, du, tm) if pk.any() else pk
    return occluded


class RayCase:
    """A scene with a ray set, the oracle's answers on it (t_ref / p_ref under the BVH,
    t_list without), its t_max sets and, computed once per set and kept, what any-hit
    must return there (`expected`: leafwise; key None: t_max = +inf)."""

    def __init__(self, O, scene, o, d, keep=None):
        self.O, self.scene, self.keep = O, scene, keep
        self.view = C.pointer(scene) if isinstance(scene, _ffi.Scene) else getattr(scene, "view", scene)
        self.o = np.ascontiguousarray(o, F)
        self.d = np.ascontiguousarray(d, F)
        self.nodes = O.bvh_build(self.view)[:4]
        self.t_ref, self.p_ref = O.trace(self.view, True, self.o, self.d)
        self.t_list, _ = O.trace(self.view, False, self.o, self.d)
        self.sets = t_max_sets(self.t_ref, self.t_list)
        self._expected = {}

    def __len__(self):
        return len(self.o)

    def t_max(self, key):
        return None if key is None else self.sets[key]

    def expected(self, key):
        if key not in self._expected:
            self._expected[key] = leafwise(self.O, self.view, self.nodes, self.o, self.d, self.t_max(key))
        return self._expected[key]


SETS = ("t_ref", "next(t_ref)", "t_ref(1+2^-15)", "t_ref(1+2^-13)", "next(t_list)", "t_list(1+2^-15)", "t_ref/2",
        "2 t_ref")


def t_max_sets(t_ref, t_list, seed=0):
    """Per ray, the t_max values around the reference's own answers (dict name -> float32[n]):
    t_ref the oracle's closest t under the BVH, t_list without it.  A ray that misses gets a
    log-uniform value in [1e-2, 1e3] instead."""
    t_ref = np.asarray(t_ref, F)
    t_list = np.asarray(t_list, F)
    rng = np.random.default_rng(seed)
    fill = (10.0 ** rng.uniform(-2, 3, len(t_ref))).astype(F)
    a = np.where(np.isfinite(t_ref), t_ref, fill).astype(F)
    b = np.where(np.isfinite(t_list), t_list, fill).astype(F)
    inf = F(np.inf)
    return {
        "t_ref": a,
        "next(t_ref)": np.nextafter(a, inf),
        "t_ref(1+2^-15)": (a * F(1 + 2.0 ** -15)).astype(F),
        "t_ref(1+2^-13)": (a * F(1 + 2.0 ** -13)).astype(F),
        "next(t_list)": np.nextafter(b, inf),
        "t_list(1+2^-15)": (b * F(1 + 2.0 ** -15)).astype(F),
        "t_ref/2": (a * F(0.5)).astype(F),
        "2 t_ref": (a * F(2)).astype(F),
    }
