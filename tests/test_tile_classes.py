"""The conservative tile classifier (tile_class.cpp, zrt_debug_tile_classes; no device).

A tile classed sky renders in a kernel that traces nothing, so the classifier must
never call a tile sky when any primary ray the kernels can generate for it returns a
hit from the reference's closest-hit query.  Checked here against the oracle's own
trace (oracle_trace) with the kernels' ray arithmetic redone in f32:

  u = (px + r - 0.5) / width, v = (py + r' - 0.5) / height, r, r' in [0, 1)
  d = llc + hor u + ver v - origin        (Camera.getRay; oracle_trace normalises)

for the footprint's corners and edge midpoints (r = 0 and the largest r below 1) and
64 random jitters per pixel.  "general" is always a safe answer, so the tests also ask
that the classifier is not vacuous: sky tiles border tiles with hits, and the bench
frame keeps a sky share of at least 0.30.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import lean_scenes as LS

F = np.float32
R_MAX = np.nextafter(F(1.0), F(0.0))  # the largest r below 1
SKY = z.ZRT_TILE_SKY


def clear_knob(monkeypatch):
    monkeypatch.delenv("ZRT_SKY_TILES", raising=False)


def cam_vecs(cam):
    v = lambda a: np.array([a.x, a.y, a.z], F)
    return v(cam.origin), v(cam.lower_left_corner), v(cam.horizontal), v(cam.vertical)


def primary_rays(cam, width, height, px, py, rx, ry):
    """Camera.getRay's unnormalised direction in f32, op by op as render.hip has it."""
    o, llc, hor, ver = cam_vecs(cam)
    u = ((px.astype(F) + rx.astype(F)) - F(0.5)) / F(width)
    v = ((py.astype(F) + ry.astype(F)) - F(0.5)) / F(height)
    d = ((llc[None, :] + hor[None, :] * u[:, None]) + ver[None, :] * v[:, None]) - o[None, :]
    return np.broadcast_to(o, d.shape).copy(), d.astype(F)


def tile_pixels(t, tiles_x, xbound, height):
    x0, y0 = (t % tiles_x) * 8, (t // tiles_x) * 8
    xs, ys = np.meshgrid(np.arange(x0, min(x0 + 8, xbound)), np.arange(y0, min(y0 + 8, height)))
    return xs.ravel(), ys.ravel()


def tile_hits(view, cam, width, height, tiles, n_jit, seed):
    """Per tile of `tiles` (global ids): whether the oracle finds a hit among the tile's
    extreme jitters (r in {0, 0.5, R_MAX} on both axes) and n_jit random ones per pixel."""
    xbound, tiles_x = height, (height + 7) // 8
    rng = np.random.default_rng(seed)
    ext = np.array([(a, b) for a in (F(0), F(0.5), R_MAX) for b in (F(0), F(0.5), R_MAX)], F)
    PX, PY, RX, RY, T = [], [], [], [], []
    for t in tiles:
        xs, ys = tile_pixels(t, tiles_x, xbound, height)
        n = len(xs)
        jit = np.concatenate([np.tile(ext, (n, 1)), rng.random((n * n_jit, 2), dtype=F)])
        PX.append(np.concatenate([np.repeat(xs, len(ext)), np.repeat(xs, n_jit)]))
        PY.append(np.concatenate([np.repeat(ys, len(ext)), np.repeat(ys, n_jit)]))
        RX.append(jit[:, 0])
        RY.append(jit[:, 1])
        T.append(np.full(len(jit), t))
    if not T:
        return {}
    px, py, rx, ry, tt = (np.concatenate(a) for a in (PX, PY, RX, RY, T))
    o, d = primary_rays(cam, width, height, px, py, rx, ry)
    _, prim = O.trace(view, True, o, d)
    hit = prim >= 0
    return {int(t): bool(hit[tt == t].any()) for t in tiles}


def global_classes(view, cam, p, world=1):
    """classes per GLOBAL tile, gathered from every rank's zrt_debug_tile_classes."""
    n_tiles = ((p.height + 7) // 8) ** 2
    out = np.zeros(n_tiles, np.uint32)
    margins = None
    for rank in range(world):
        cls, margins = z.debug_tile_classes(view, cam, dataclasses.replace(p, rank=rank, world_size=world))
        assert len(cls) == len(range(rank, n_tiles, world))
        out[rank::world] = cls
    assert set(np.unique(out)) <= {0, SKY}
    return out, margins


@pytest.fixture(scope="module")
def bunny_256(scenes):
    """Scene 2 at 256 x 256: its classes, and per tile whether a pixel-centre ray hits."""
    s = scenes(2)
    cls, _ = z.debug_tile_classes(s, s.camera, z.RenderParams(256, 256, 4, 20))
    px, py = np.meshgrid(np.arange(256), np.arange(256))
    px, py = px.ravel(), py.ravel()
    half = np.full(len(px), 0.5, F)
    o, d = primary_rays(s.camera, 256, 256, px, py, half, half)
    _, prim = O.trace(s.view, True, o, d)
    hit = np.zeros(32 * 32, bool)
    np.logical_or.at(hit, (py // 8) * 32 + px // 8, prim >= 0)
    return cls, hit


@pytest.mark.parametrize("which", [0, 2, 3, 4])
@pytest.mark.parametrize("size", [(256, 256), (70, 50)])
def test_no_ray_of_a_sky_tile_hits(scenes, which, size, monkeypatch):
    clear_knob(monkeypatch)
    s = scenes(which)
    w, h = size
    p = z.RenderParams(w, h, 4, 20)
    cls, m = global_classes(s.view, s.camera, p)
    sky = np.nonzero(cls == SKY)[0]
    hits = tile_hits(s.view, s.camera, w, h, sky, 64, seed=which)
    bad = [t for t, hh in hits.items() if hh]
    assert not bad, f"scene {which} {w}x{h}: sky tiles {bad[:8]} have rays the oracle hits (margins {m})"
    if which == 2:  # (70 x 50 renders the left 50 columns only: little sky there)
        assert len(sky) > (0.25 * len(cls) if w == 256 else 0), (len(sky), len(cls))


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_classify_their_own_tiles(scenes, world, bunny_256, monkeypatch):
    """Ranks 0 .. world-1 together give the classes one rank gives (sound, then, as above)."""
    clear_knob(monkeypatch)
    s = scenes(2)
    cls, _ = global_classes(s.view, s.camera, z.RenderParams(256, 256, 4, 20), world)
    one, hit = bunny_256
    assert not (hit & (cls == SKY)).any()
    # (ranks split the frame into other blocks than one rank does: the same tiles up to
    # the few a coarser or finer cone decides differently)
    assert abs(int((cls == SKY).sum()) - int((one == SKY).sum())) <= 8
    assert ((cls == SKY) != (one == SKY)).sum() <= 16


def test_sky_tiles_border_hit_tiles_and_share(scenes, bunny_256, monkeypatch):
    clear_knob(monkeypatch)
    cls, hit = bunny_256
    sky = (cls == SKY).reshape(32, 32)
    hit = hit.reshape(32, 32)
    assert not (sky & hit).any()
    near = np.zeros_like(hit)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            sh = np.roll(np.roll(hit, dy, 0), dx, 1)
            if dy == 1: sh[0] = False
            if dy == -1: sh[-1] = False
            if dx == 1: sh[:, 0] = False
            if dx == -1: sh[:, -1] = False
            near |= sh
    assert (sky & near).any(), "no sky tile borders a tile with a hit: the margin is vacuous"
    s = scenes(2)
    big, m = z.debug_tile_classes(s, s.camera, z.RenderParams(2048, 2048, 1024, 20))
    share = float((big == SKY).mean())
    print("scene 2 at 2048^2: sky share", share, "margins", m)
    assert share >= 0.30, share


# ---- a synthetic family at the classifier's edge ----
def build_scene(prims):
    """A zrt_scene of one Lambertian colour: prims = [("s", centre, r) | ("t", a, b, c)]."""
    texs = (_ffi.Texture * 1)(_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0.5, 0.5, 0.5), 0.0, 0.0))
    mats = (_ffi.Material * 1)(_ffi.Material(_ffi.ZRT_MAT_LAMBERTIAN, 0, 0.0))
    arr = (_ffi.Prim * len(prims))()
    for i, q in enumerate(prims):
        arr[i].material = 0
        if q[0] == "s":
            arr[i].kind = _ffi.ZRT_PRIM_SPHERE
            arr[i].center = _ffi.Vec3(*[float(x) for x in q[1]])
            arr[i].radius = float(q[2])
        else:
            arr[i].kind = _ffi.ZRT_PRIM_TRIANGLE
            arr[i].a, arr[i].b, arr[i].c = (_ffi.Vec3(*[float(x) for x in v]) for v in q[1:4])
    s = _ffi.Scene(arr, len(prims), 1, mats, texs, 1, 0, C.cast(None, C.POINTER(_ffi.Image)))
    s._keep = (arr, mats, texs)
    return s


def edge_direction(cam, width, height, x_edge, y):
    """The exact direction through frame position (x_edge, y) in jitter units (f64)."""
    o, llc, hor, ver = (a.astype(np.float64) for a in cam_vecs(cam))
    d = llc + hor * (x_edge / width) + ver * (y / height) - o
    return o, d / np.linalg.norm(d)


def family(kind):
    """16 primitives, each beside the right edge of its own tile (tiles (2 + 4i, 2 + 4j) of a
    128 x 128 frame), its nearest point offset from the edge by f x its reach, f = 0.25
    (the reach enters the tile's footprint) or 3 (it stays outside)."""
    cam = z.camera_init((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 40.0, 1.0)
    rng = np.random.default_rng(5 if kind == "s" else 6)
    prims, where = [], []
    for i in range(4):
        for j in range(4):
            tx, ty = 2 + 4 * i, 2 + 4 * j
            f = 0.25 if (i + j) % 2 == 0 else 3.0
            x_edge = 8.0 * (tx + 1) - 0.5  # the largest px + r - 0.5 of the tile
            o, d = edge_direction(cam, 128, 128, x_edge, 8.0 * ty + 4.0)
            right = np.cross(d, np.array([0.0, 1.0, 0.0]))
            right /= np.linalg.norm(right)
            if right[0] < 0:
                right = -right
            if kind == "s":  # small far spheres (tests/adversarial_rays.py's kind)
                dist, r = float(rng.uniform(40.0, 150.0)), float(rng.uniform(0.005, 0.5))
                E = 32.0 * 2.0 ** -24 * (dist * dist + r * r)
                reach = np.sqrt(E)  # what the rounded test can reach past the surface
                c = o + d * dist + right * (r + f * reach)
                prims.append(("s", c, r))
            else:  # thin triangles seen almost edge-on (tests/grazing_tris.py's kind)
                dist, size = float(rng.uniform(5.0, 20.0)), float(rng.uniform(0.005, 0.02))
                tilt = float(rng.uniform(1e-3, 3e-2))  # the plane's angle to the ray
                n = right * np.cos(tilt) - d * np.sin(tilt)  # faces the camera, barely
                e1 = np.cross(n, np.array([0.0, 1.0, 0.0]))
                e1 /= np.linalg.norm(e1)
                e2 = np.cross(e1, n)
                reach = 2.6 * 2.0 ** -24 * dist * size * size / (size * size * np.sin(tilt) + 1e-30)
                a = o + d * dist + right * (f * reach)
                b, c = a + e1 * size + right * 1e-4, a + e2 * size + right * 1e-4
                if np.dot(np.cross(b - a, c - a), d) > 0:  # single sided: det = -d . n >= 1e-6
                    b, c = c, b
                prims.append(("t", a, b, c))
            where.append((ty * 16 + tx, f))
    return cam, build_scene(prims), where


@pytest.mark.parametrize("kind", ["s", "t"])
def test_synthetic_edge_family(kind, monkeypatch):
    """No tile in which the oracle finds a hit is classed sky, in a scene built to put a
    primitive's reach just inside and just outside tile footprints; the frame is not all
    general, and every tile a primitive's reach enters is general."""
    clear_knob(monkeypatch)
    cam, s, where = family(kind)
    view = C.pointer(s)
    p = z.RenderParams(128, 128, 4, 20)
    cls, m = z.debug_tile_classes(view, cam, p)
    assert len(cls) == 256
    hits = tile_hits(view, cam, 128, 128, range(256), 64, seed=9)
    bad = [t for t in range(256) if hits[t] and cls[t] == SKY]
    assert not bad, (kind, bad, m)
    assert (cls == SKY).sum() > 128, "the family's frame is mostly empty sky"
    for t, f in where:
        if f < 1.0:
            assert cls[t] != SKY, (kind, t, m)
        assert cls[t + 1] != SKY  # (the tile the primitive itself lies in)
    print(kind, "hit tiles", sum(hits.values()), "sky tiles", int((cls == SKY).sum()), "margins", m)


# ---- eligibility, swept like tests/test_lean_kernel.py ----
@pytest.mark.parametrize("which", [1, 2, 3, "a", "d"])
def test_split_eligibility(scenes, which, monkeypatch):
    """Depth 0, 1, 20 x flags x traversal x ZRT_SKY_TILES unset, 0, 1: a sky tile is
    reported only for the lockstep FAST loop with depth >= 1, without SCANLINES and
    GUARD, from a camera inside the origin bound, and never under ZRT_SKY_TILES=0."""
    if which in LS.NAMES:
        keep, view, cam = LS.get(which)
        inside = which != "d"
    else:
        s = scenes(which)
        view, cam, inside = s.view, s.camera, True
    n_split = 0
    for depth in (0, 1, 20):
        for flags in (0, z.ZRT_FLAG_SCANLINES, z.ZRT_FLAG_GUARD, z.ZRT_FLAG_STATS):
            for trav in (z.ZRT_TRAVERSAL_FAST, z.ZRT_TRAVERSAL_REFERENCE, z.ZRT_TRAVERSAL_BINARY):
                p = z.RenderParams(64, 64, 4, depth, flags=flags, traversal=trav)
                monkeypatch.delenv("ZRT_SKY_TILES", raising=False)
                plan = z.debug_launch_plan(view, p)
                eligible = (plan["kmode"] == 3 and depth >= 1 and inside
                            and not flags & (z.ZRT_FLAG_SCANLINES | z.ZRT_FLAG_GUARD))
                counts = {}
                for knob in (None, "0", "1"):
                    if knob is None:
                        monkeypatch.delenv("ZRT_SKY_TILES", raising=False)
                    else:
                        monkeypatch.setenv("ZRT_SKY_TILES", knob)
                    cls, _ = z.debug_tile_classes(view, cam, p)
                    counts[knob] = int((cls == SKY).sum())
                where = f"scene {which} depth {depth} flags {flags} traversal {trav}: {counts}"
                assert counts["0"] == 0, where
                assert counts[None] == counts["1"], where  # the default is on
                if not eligible:
                    assert counts["1"] == 0, where
                n_split += counts["1"] > 0
    if which == 2:
        assert n_split > 0, "an eligible scene never splits"
    # 1: a list of spheres (no tree); d: a camera outside the bound; 3, a: triangles whose
    # first-order reach at the det floor exceeds the camera's distance (every tile general)
    if which in (1, 3, "a", "d"):
        assert n_split == 0


def test_non_finite_plane_means_no_split(monkeypatch):
    """A scene with an infinite coordinate in a triangle: every tile general."""
    clear_knob(monkeypatch)
    cam, s, _ = family("s")
    view = C.pointer(s)
    cls, _ = z.debug_tile_classes(view, cam, z.RenderParams(128, 128, 4, 20))
    assert (cls == SKY).any()
    prims = [("s", (float(i), 0.0, -50.0), 0.1) for i in range(12)]
    prims.append(("t", (0.0, 0.0, -30.0), (1.0, 0.0, -30.0), (0.0, float("inf"), -30.0)))
    s2 = build_scene(prims)
    cls2, _ = z.debug_tile_classes(C.pointer(s2), cam, z.RenderParams(128, 128, 4, 20))
    assert not (cls2 == SKY).any()
