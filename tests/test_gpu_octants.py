"""The FAST traversal's octant handling against the oracle.

A ray reads the copy of the wide tree stored for its octant (the signs of 1/d): the
copy's offset in global memory and in the LDS top levels is octant x stride, formed by
a 24-bit multiply, and the three sign masks themselves are formed only where a rare
path reads them (the order-hazard replay's box test; the per-axis tests of loose_slot
and static_ok_slot run on the octant copy's pre-swapped planes).

1. Frames: scenes 2 and 3 at 32 x 32 x 4, depths 1 and 6, both generators, the lean
   and the general kernel: the oracle's frame bit for bit and its Progress counters.
2. zrt_trace on the ray sets that drive those rare paths - tests/grazing_rays.py on
   scenes 2 and 3, tests/hazard_rays.py - with scene and rays mirrored into each of the
   eight octants (sign flips are exact in f32, so every coincidence of a ray with a box
   plane survives the mirror; a triangle's b and c are swapped under an odd number of
   flips, which keeps its facing): surface and t equal the oracle's on every ray.

Run on an MI355X: ``pytest -m gpu``.
"""
import ctypes as C

import numpy as np
import pytest

import zraytrace_amd as z
from oracle import oracle_py as O
from zraytrace_amd import _ffi

import grazing_rays as G
import hazard_rays as H
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

PRNGS = {"xoroshiro": z.ZRT_PRNG_XOROSHIRO128, "xoshiro": z.ZRT_PRNG_XOSHIRO256}
_ORACLE = {}
_RAYS = {}


def lockstep(monkeypatch):
    for k in ("ZRT_WF", "ZRT_POOL", "ZRT_QNODES", "ZRT_LIST_LANES", "ZRT_ATT_LDS_ROWS"):
        monkeypatch.delenv(k, raising=False)


# ---- 1. frames ------------------------------------------------------------------------------

def oracle_frame(which, view, cam, p):
    k = (which, p.max_depth, p.prng)
    if k not in _ORACLE:
        img, st = O.render(view, cam, p)
        img.setflags(write=False)
        _ORACLE[k] = (img, st)
    return _ORACLE[k]


@pytest.mark.parametrize("knob", ["1", "0"])
@pytest.mark.parametrize("prng", list(PRNGS))
@pytest.mark.parametrize("max_depth", [1, 6])
@pytest.mark.parametrize("which", [2, 3])
def test_frames_equal_the_oracle(scenes, which, max_depth, prng, knob, monkeypatch):
    lockstep(monkeypatch)
    monkeypatch.setenv("ZRT_LEAN", knob)
    s = scenes(which)
    p = z.RenderParams(32, 32, 4, max_depth, prng=PRNGS[prng])
    assert z.debug_lean_kernel(s.view, s.camera, p) == (knob == "1")
    ref, rs = oracle_frame(which, s.view, s.camera, p)
    gpu, gs = z.render(s, s.camera, p)
    P.assert_bit_exact(gpu, ref)
    for k in P.COUNTERS:
        assert gs[k] == rs[k], k
    assert gs["sampling_loop"] == 3
    # (camera rays of this frame leave in more than one octant, scattered rays in all eight)
    assert rs["reflections"] > 0


# ---- 2. zrt_trace, mirrored into every octant --------------------------------------------------

def mirrored_scene(view, signs):
    """The scene with every coordinate multiplied by signs (each +-1), all black metal."""
    v = view.contents if hasattr(view, "contents") else view
    src = P.prim_array(v)
    n = v.n_prims
    prims = (_ffi.Prim * n)()
    dst = np.frombuffer((C.c_uint8 * C.sizeof(prims)).from_address(C.addressof(prims)), dtype=src.dtype)
    sg = np.asarray(signs, np.float32)
    dst["kind"] = src["kind"]
    dst["material"] = 0
    dst["radius"] = src["radius"]
    dst["center"] = src["center"] * sg
    odd = float(np.prod(signs)) < 0
    dst["a"] = src["a"] * sg
    dst["b"] = src["c" if odd else "b"] * sg
    dst["c"] = src["b" if odd else "c"] * sg
    texs = (_ffi.Texture * 1)(_ffi.Texture(_ffi.ZRT_TEX_COLOR, 0, _ffi.Vec3(0, 0, 0), 0.0, 0.0))
    mats = (_ffi.Material * 1)(_ffi.Material(_ffi.ZRT_MAT_METAL, 0, 0.0))
    scene = _ffi.Scene(prims, n, 1, mats, texs, 1, 0, C.cast(None, C.POINTER(_ffi.Image)))
    scene._keep = (prims, mats, texs)
    return scene


def ray_set(scenes, which):
    """(scene view, origins, directions) in the scene's own orientation, built once."""
    if which not in _RAYS:
        if which == "hazard":
            view, o, d = H.hazard_scene(1, 60000)
        else:
            view = scenes(which).view
            pr = P.prim_array(view.contents)
            mins, maxs, left, _, _ = O.bvh_build(view)
            o, d = G.grazing_rays(pr, mins, maxs, left, n=3000, seed=7, span=float(np.max(maxs[0] - mins[0])))
        o.setflags(write=False)
        d.setflags(write=False)
        _RAYS[which] = (view, o, d)
    return _RAYS[which]


@pytest.mark.parametrize("octant", range(8))
@pytest.mark.parametrize("which", [2, 3, "hazard"])
def test_trace_mirrored_equals_the_oracle(scenes, which, octant):
    view, o, d = ray_set(scenes, which)
    signs = [-1.0 if octant >> k & 1 else 1.0 for k in range(3)]
    sg = np.asarray(signs, np.float32)
    scene = mirrored_scene(view, signs)
    om, dm = np.ascontiguousarray(o * sg), np.ascontiguousarray(d * sg)
    t_ref, p_ref = O.trace(scene, True, om, dm)
    assert (p_ref >= 0).mean() > 0.5
    if which == "hazard" and octant == 0:  # (the set does what it is for: the DFS order decides some rays)
        _, p_list = O.trace(scene, False, om, dm)
        assert (p_ref != p_list).sum() > 40
    t, p = z.trace(scene, z.RenderParams(1, 1, 1, 1, traversal=z.ZRT_TRAVERSAL_FAST), om, dm)
    P.assert_same_hits(t, p, t_ref, p_ref)
    # every octant of 1/d occurs among the rays (zero components count as positive)
    octs = (dm[:, 0] < 0) * 1 + (dm[:, 1] < 0) * 2 + (dm[:, 2] < 0) * 4
    if which != "hazard":
        assert len(np.unique(octs)) == 8
