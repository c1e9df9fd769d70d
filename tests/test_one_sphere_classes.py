"""The one-sphere tile class (tile_class.cpp, zrt_debug_tile_classes; no device).

A tile classed one-sphere(s) renders in a kernel whose camera rays test the sphere s
alone, so the classifier must never give a tile that class when a primary ray the
kernels can generate for it returns a hit on another primitive from the reference's
closest-hit query.  Checked against the oracle's own trace with tests/test_tile_classes.py's
ray generator: the footprint's corners, edge midpoints and centre, and random jitters.
"general" is always a safe answer, so the share of scene 2's ground-only tiles that get
the class is asked for too (0.9 of the tiles the oracle's first hits leave after eroding
two tiles: the ground sphere's reach is larger than the sky class's margins).

The class word is ZRT_TILE_ONE_SPHERE | the sphere's device primitive slot s; every
one-sphere tile of a call names the same sphere.  The oracle reports list indices;
zrt_debug_slot_prims maps the slot onto one, so every hit in a tile is asked to be on the
primitive its own class word names, a sphere.
"""
import dataclasses

import numpy as np
import pytest

import zraytrace_amd as z
from zraytrace_amd import _ffi
from oracle import oracle_py as O

import lean_scenes as LS
import sphere_scenes as SS
import test_tile_classes as TC

F = np.float32
SKY, ONE = z.ZRT_TILE_SKY, z.ZRT_TILE_ONE_SPHERE
N_JIT = 24  # random jitters per pixel, besides the nine extreme ones


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in ("ZRT_SKY_TILES", "ZRT_SPHERE_TILES", "ZRT_LEAN", "ZRT_WF", "ZRT_POOL", "ZRT_QNODES"):
        monkeypatch.delenv(k, raising=False)


def is_one(cls):
    return ((cls & SKY) == 0) & ((cls & ONE) != 0)


def global_classes(view, cam, p, world=1):
    """Class words per GLOBAL tile, gathered from every rank's call; a rank's one-sphere
    tiles all name one sphere, and the default view of the same call shows them general."""
    n_tiles = ((p.height + 7) // 8) ** 2
    out = np.zeros(n_tiles, np.uint32)
    for rank in range(world):
        pr = dataclasses.replace(p, rank=rank, world_size=world)
        cls, _ = z.debug_tile_classes(view, cam, pr, one_sphere=True)
        assert len(cls) == len(range(rank, n_tiles, world))
        assert len(np.unique(cls[is_one(cls)])) <= 1
        plain, _ = z.debug_tile_classes(view, cam, pr)
        assert set(np.unique(plain)) <= {0, SKY}
        np.testing.assert_array_equal(plain == SKY, cls == SKY)
        out[rank::world] = cls
    assert set(np.unique(out[~is_one(out)])) <= {0, SKY}
    return out


def tile_prims(view, cam, width, height, tiles, n_jit, seed, extremes=True):
    """Per tile of `tiles` (global ids): the set of list indices the oracle's closest-hit
    query returns over the tile's extreme jitters (extremes False: the pixel centres alone)
    and n_jit random ones per pixel (-1: a miss)."""
    xbound, tiles_x = height, (height + 7) // 8
    rng = np.random.default_rng(seed)
    ext = np.array([(a, b) for a in (F(0), F(0.5), TC.R_MAX) for b in (F(0), F(0.5), TC.R_MAX)], F)
    if not extremes:
        ext = np.array([(F(0.5), F(0.5))], F)
    PX, PY, RX, RY, T = [], [], [], [], []
    for t in tiles:
        xs, ys = TC.tile_pixels(t, tiles_x, xbound, height)
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
    o, d = TC.primary_rays(cam, width, height, px, py, rx, ry)
    _, prim = O.trace(view, True, o, d)
    order = np.argsort(tt, kind="stable")
    tt, prim = tt[order], prim[order]
    cut = np.nonzero(np.diff(tt))[0] + 1
    return {int(g[0]): set(int(x) for x in np.unique(q)) for g, q in zip(np.split(tt, cut), np.split(prim, cut))}


def assert_sound(view, p, cls, prims, where):
    """Every hit in a one-sphere tile of `cls` is on the primitive in the device slot the
    tile's class word names (zrt_debug_slot_prims), a sphere.  Returns the primitives hit."""
    slot_prim = z.debug_slot_prims(view, p)
    seen = set()
    for t in np.nonzero(is_one(cls))[0]:
        slot = int(cls[t]) & (ONE - 1)
        assert slot < len(slot_prim), (where, t, hex(cls[t]))
        s = int(slot_prim[slot])
        assert view.contents.prims[s].kind == _ffi.ZRT_PRIM_SPHERE, (where, t, slot, s)
        other = prims[int(t)] - {-1, s}
        assert not other, f"{where}: tile {t} is one-sphere({s}, slot {slot}) but its rays hit {sorted(other)[:8]}"
        seen |= prims[int(t)] - {-1}
    return seen


# ---- soundness on the reference scenes ----
@pytest.mark.parametrize("which", [0, 2, 3, 4])
@pytest.mark.parametrize("size", [(256, 256), (70, 50)])
def test_no_ray_of_a_one_sphere_tile_hits_another_primitive(scenes, which, size):
    s = scenes(which)
    w, h = size
    p = z.RenderParams(w, h, 4, 20)
    per_world = {world: global_classes(s.view, s.camera, p, world) for world in (1, 2, 3)}
    tiles = sorted(set(int(t) for cls in per_world.values() for t in np.nonzero(is_one(cls))[0]))
    prims = tile_prims(s.view, s.camera, w, h, tiles, N_JIT, seed=which)
    for world, cls in per_world.items():
        assert not (is_one(cls) & (cls == SKY)).any()
        seen = assert_sound(s.view, p, cls, prims, f"scene {which} {w}x{h} world {world}")
        if which == 2:
            assert seen == {SS.sphere_indices(s.view)[0]}  # the ground sphere
            assert is_one(cls).sum() > 0.3 * len(cls), (world, int(is_one(cls).sum()))
        print(f"scene {which} {w}x{h} world {world}: {int(is_one(cls).sum())} one-sphere, "
              f"{int((cls == SKY).sum())} sky of {len(cls)}")


def erode2(mask):
    """A tile survives when every tile within two of it (inside the frame) is set."""
    n = mask.shape[0]
    out = mask.copy()
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            sh = np.ones_like(mask)
            ys, xs = slice(max(0, dy), n + min(0, dy)), slice(max(0, dx), n + min(0, dx))
            yd, xd = slice(max(0, -dy), n + min(0, -dy)), slice(max(0, -dx), n + min(0, -dx))
            sh[yd, xd] = mask[ys, xs]
            out &= sh
    return out


def test_share_of_the_ground_only_tiles(scenes):
    """Scene 2 at 256 x 256: of the tiles whose sampled rays hit the ground sphere or
    nothing, with at least one hit, eroded by two tiles, the classifier gives 0.9 the class."""
    s = scenes(2)
    p = z.RenderParams(256, 256, 4, 20)
    cls = global_classes(s.view, s.camera, p)
    ground = SS.sphere_indices(s.view)[0]
    # (the pixel centres first: the oracle is slow on the bunny, and a tile with a centre
    # on it is out already; the others take the extreme jitters and eight random ones)
    prims = tile_prims(s.view, s.camera, 256, 256, range(1024), 0, seed=21, extremes=False)
    rest = [t for t in range(1024) if prims[t] <= {ground, -1}]
    for t, q in tile_prims(s.view, s.camera, 256, 256, rest, 8, seed=21).items():
        prims[t] |= q
    only = np.array([prims[t] <= {ground, -1} and ground in prims[t] for t in range(1024)]).reshape(32, 32)
    eroded = erode2(only)
    got = int(is_one(cls).sum())
    print(f"scene 2 at 256^2: {got} one-sphere tiles; the oracle's ground-only tiles {int(only.sum())}, "
          f"eroded by two {int(eroded.sum())}")
    assert got >= 0.9 * int(eroded.sum()), (got, int(eroded.sum()))


# ---- eligibility ----
def counts(view, cam, p):
    cls, _ = z.debug_tile_classes(view, cam, p, one_sphere=True)
    return cls, int(is_one(cls).sum())


def test_ineligible_launches_have_no_one_sphere_tile(scenes, monkeypatch):
    """Depth 0, SCANLINES, GUARD, a dielectric or an image texture in the table, a camera
    outside the origin bound, a list scene, ZRT_SPHERE_TILES=0: no one-sphere tile, and the
    sky classes of a run with ZRT_SPHERE_TILES=0.  (Each beside the eligible launch it
    differs from in that one condition, which does have one-sphere tiles.)"""
    _, view, cam = SS.get("horizon")
    base = z.RenderParams(64, 64, 4, 20)
    cases = [("eligible", view, cam, base, True),
             ("stats", view, cam, dataclasses.replace(base, flags=z.ZRT_FLAG_STATS), True),
             ("depth 1", view, cam, dataclasses.replace(base, max_depth=1), True),
             ("depth 0", view, cam, dataclasses.replace(base, max_depth=0), False),
             ("scanlines", view, cam, dataclasses.replace(base, flags=z.ZRT_FLAG_SCANLINES), False),
             ("guard", view, cam, dataclasses.replace(base, flags=z.ZRT_FLAG_GUARD), False),
             ("reference traversal", view, cam, dataclasses.replace(base, traversal=z.ZRT_TRAVERSAL_REFERENCE), False),
             ("dielectric", SS.get("horizon", "dielectric")[1], cam, base, False),
             ("image texture", SS.get("horizon", "image")[1], cam, base, False),
             ("camera outside", view, z.camera_init((0.0, 450.0, 0.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), 20.0, 1.0),
              base, False),
             ("list scene", scenes(1).view, scenes(1).camera, base, False),
             ("lean scene d", LS.get("d")[1], LS.get("d")[2], base, False)]
    for name, v, c, p, eligible in cases:
        monkeypatch.delenv("ZRT_SPHERE_TILES", raising=False)
        cls_on, n_on = counts(v, c, p)
        monkeypatch.setenv("ZRT_SPHERE_TILES", "1")
        assert counts(v, c, p)[1] == n_on, name  # the default is on
        monkeypatch.setenv("ZRT_SPHERE_TILES", "0")
        cls_off, n_off = counts(v, c, p)
        assert n_off == 0, name
        np.testing.assert_array_equal(cls_on == SKY, cls_off == SKY, err_msg=name)
        if eligible:
            assert n_on > 0, name
        else:
            assert n_on == 0, name
            np.testing.assert_array_equal(cls_on, cls_off, err_msg=name)
    monkeypatch.setenv("ZRT_SPHERE_TILES", "1")
    monkeypatch.setenv("ZRT_SKY_TILES", "0")  # (the class rides on the sky split)
    assert counts(view, cam, base)[1] == 0
    monkeypatch.delenv("ZRT_SKY_TILES")
    monkeypatch.setenv("ZRT_LEAN", "0")  # (no lean kernel, no one-sphere kernel)
    assert counts(view, cam, base)[1] == 0


# ---- synthetic scenes ----
def synthetic(name, w=64, h=64):
    _, view, cam = SS.get(name)
    p = z.RenderParams(w, h, 4, 20)
    cls = global_classes(view, cam, p)
    prims = tile_prims(view, cam, w, h, range(len(cls)), N_JIT, seed=5)
    seen = assert_sound(view, p, cls, prims, name)
    return view, cls, prims, seen


def test_horizon_tiles_are_one_sphere():
    view, cls, prims, seen = synthetic("horizon")
    ground = SS.sphere_indices(view)[0]
    assert seen == {ground}
    horizon = [t for t in range(64) if prims[t] == {ground, -1}]  # tiles whose rays both hit and miss
    assert len(horizon) >= 6, horizon
    assert all(is_one(cls)[t] for t in horizon), [(t, hex(cls[t])) for t in horizon]
    assert (cls == 0).any() and (cls == SKY).any()  # the cluster's tiles, the sky above


def test_overlapping_spheres_leave_the_overlap_general():
    view, cls, prims, seen = synthetic("overlap")
    a, b = SS.sphere_indices(view)[:2]
    both = [t for t in range(64) if {a, b} <= prims[t]]
    assert both and all(cls[t] == 0 for t in both), [(t, hex(cls[t])) for t in both]
    assert is_one(cls).any() and len(seen) == 1


def test_a_sphere_behind_the_camera_is_never_the_one():
    view, cls, prims, seen = synthetic("behind")
    ground = SS.sphere_indices(view)[0]
    assert seen == {ground} and is_one(cls).sum() >= 24
    # ... and with the ground gone, the frame is sky but for the cluster: no tile names the sphere behind
    s2 = SS.build([("s", (0.0, 1.0, 8.0), 2.0)] + SS.cluster((3.0, 2.5, -12.0)))
    import ctypes as C
    cls2, _ = z.debug_tile_classes(C.pointer(s2), SS.get("behind")[2], z.RenderParams(64, 64, 4, 20), one_sphere=True)
    assert not is_one(cls2).any()


def test_a_camera_inside_a_sphere_is_sound():
    view, cls, prims, seen = synthetic("inside")
    assert set(np.unique(cls[~is_one(cls)])) <= {0}  # no sky from inside
    assert (cls == 0).any()  # the cluster's tiles


def test_two_disjoint_spheres_keep_the_one_with_more_tiles():
    view, cls, prims, seen = synthetic("two")
    big, small = SS.sphere_indices(view)[:2]
    assert seen == {big}
    only_small = [t for t in range(64) if prims[t] - {-1} == {small}]
    assert only_small and all(cls[t] == 0 for t in only_small)
    assert is_one(cls).sum() > len(only_small)


@pytest.mark.parametrize("name,w", [("all", 64), ("down_z", 65), ("slit", 64)])
def test_other_gpu_scenes_are_sound(name, w):
    """The scenes tests/test_gpu_sphere_tiles.py renders besides: sound, and not vacuous."""
    view, cls, prims, seen = synthetic(name, w, 64)
    assert is_one(cls).sum() >= (64 if name == "all" else 24)
